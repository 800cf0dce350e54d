// mi355dr.hip -- host side of libmi355dr.so: the C ABI declared in include/mi355dr.h, device-memory
// management, and the launch schedule of the search (chunked screen -> prune, exact fallback).
// gfx950 only.  Build: see __graft_entry__.build().
#include "index.h"
#include "k_prep.h"
#include "k_scan.h"
#include "k_scan_ids.h"
#include "subset_ids.h"
#include "screen_common.h"
#include "k_screen.h"
#include "k_screen256c.h"
#include "k_screen_rq.h"

// K-step counts k_screen_rq is built for (int8 shadow rows of 128 ... 768 bytes)
#define MI355_RQ_FORMS(X) X(1) X(2) X(3) X(4) X(5) X(6)
inline bool screen_rq_has(int ksteps) { return ksteps >= 1 && ksteps <= 6; }
#include "k_screen_stream.h"
#include "k_select.h"
#include "k_prune_wide.h"
#include "k_update.h"
#include "k_compact.h"
#include "k_view.h"
#include "k_block.h"
#include "k_mmr.h"
#include "mmr_order.h"
#include "k_groups.h"
#include "k_fuse.h"
#include "k_collapse.h"
#include "collapse_plan.h"
#include "k_range.h"
#include "k_rows.h"
#include "k_combine.h"
#include "k_shard.h"

#include <functional>

using namespace mi355;

namespace {
std::mutex g_err_mu;
std::string g_err;  // errors raised before a handle exists
}  // namespace

namespace mi355 {
int fail(mi355dr_index* idx, int code, const std::string& msg) {
    if (idx) idx->err = msg;
    else {
        std::lock_guard<std::mutex> g(g_err_mu);
        g_err = msg;
    }
    return code;
}
}  // namespace mi355

namespace {


int ensure_capacity(mi355dr_index* idx, int64_t want_rows) {
    if (want_rows <= idx->cap_rows) return MI355DR_OK;
    int64_t new_cap = std::max<int64_t>(want_rows, idx->cap_rows + idx->cap_rows / 2);
    new_cap = round_up(std::max<int64_t>(new_cap, kT2), kT2);  // whole 256-row screen tiles
    // the new blocks live in local owners until the swap: a failure on the way leaves the index as it was and leaks nothing
    DevBuf<float> rows, nrm2;
    DevBuf<uint16_t> shadow;
    DevBuf<int8_t> shadow8;
    DevBuf<uint8_t> flag8;
    DevBuf<I8Group> grp8;
    const size_t row_b = (size_t)idx->dim * sizeof(float), sh_b = (size_t)idx->dpad * sizeof(uint16_t), sh8_b = (size_t)idx->dpad8;
    const size_t grp_b = (size_t)(new_cap / kI8GroupRows) * sizeof(I8Group);
    HIPCHECK(idx, rows.grow(new_cap * row_b));
    HIPCHECK(idx, shadow.grow(new_cap * sh_b));
    HIPCHECK(idx, nrm2.grow(new_cap * sizeof(float)));
    HIPCHECK(idx, shadow8.grow(new_cap * sh8_b));
    HIPCHECK(idx, flag8.grow(new_cap));
    HIPCHECK(idx, grp8.grow(grp_b));
    hipStream_t s = idx->stream;
    HIPCHECK(idx, hipMemsetAsync(shadow, 0, new_cap * sh_b, s));
    HIPCHECK(idx, hipMemsetAsync(shadow8, 0, new_cap * sh8_b, s));
    HIPCHECK(idx, hipMemsetAsync(flag8, 0, new_cap, s));
    HIPCHECK(idx, hipMemsetAsync(grp8, 0, grp_b, s));
    if (idx->n > 0) {
        const size_t n = idx->n, live_grp_b = (n + kI8GroupRows - 1) / kI8GroupRows * sizeof(I8Group);
        HIPCHECK(idx, hipMemcpyAsync(rows, idx->rows, n * row_b, hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(shadow, idx->shadow, n * sh_b, hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(nrm2, idx->nrm2, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(shadow8, idx->shadow8, n * sh8_b, hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(flag8, idx->flag8, n, hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(grp8, idx->grp8, live_grp_b, hipMemcpyDeviceToDevice, s));
    }
    HIPCHECK(idx, hipStreamSynchronize(s));
    idx->rows.swap(rows);  // (the old blocks leave with the locals)
    idx->shadow.swap(shadow);
    idx->nrm2.swap(nrm2);
    idx->shadow8.swap(shadow8);
    idx->flag8.swap(flag8);
    idx->grp8.swap(grp8);
    idx->cap_rows = new_cap;
    return MI355DR_OK;
}

int ensure_qstate(mi355dr_index* idx) {
    if (idx->qstate_ready) return MI355DR_OK;
    const size_t B = kQBlockMax;
    // a view of st gets its block from the owner at the same position; grow() keeps what an earlier, failed call already got
    auto own = [&](auto*& view, size_t bytes) {
        DevBuf<void>& mem = idx->st_mem[((char*)&view - (char*)&idx->st) / sizeof(void*)];
        const hipError_t e = mem.grow(bytes);
        view = static_cast<std::remove_reference_t<decltype(view)>>(mem.p);
        return e;
    };
    HIPCHECK(idx, own(idx->st.qn, B * sizeof(float)));
    HIPCHECK(idx, own(idx->st.qhat, B * idx->dpad * sizeof(uint16_t)));
    HIPCHECK(idx, own(idx->st.thr, B * sizeof(float)));
    HIPCHECK(idx, own(idx->st.cnt, B * sizeof(int)));
    HIPCHECK(idx, own(idx->st.best_n, B * sizeof(int)));
    HIPCHECK(idx, own(idx->st.best_key, B * kKMax * sizeof(uint64_t)));
    HIPCHECK(idx, own(idx->st.best_row, B * kKMax * sizeof(int32_t)));
    HIPCHECK(idx, own(idx->st.thr_key, B * sizeof(uint64_t)));
    HIPCHECK(idx, own(idx->st.thr_row, B * sizeof(int32_t)));
    HIPCHECK(idx, own(idx->st.status, (B + 1) * sizeof(int)));  // [B]: the block's OR-ed status word
    idx->status_or_dev = idx->st.status + B;
    HIPCHECK(idx, own(idx->st.E, B * sizeof(float)));
    HIPCHECK(idx, own(idx->st.E16, B * sizeof(float)));
    HIPCHECK(idx, own(idx->st.sc, B * sizeof(float)));
    HIPCHECK(idx, own(idx->st.kq, B * sizeof(float)));
    HIPCHECK(idx, idx->rq_progress.grow(kRqProgressWords * sizeof(int)));
    HIPCHECK(idx, hipMemset(idx->rq_progress, 0, kRqProgressWords * sizeof(int)));
    HIPCHECK(idx, own(idx->st.qhat8, B * idx->dpad8));
    HIPCHECK(idx, own(idx->st.carry, B * sizeof(int)));
    HIPCHECK(idx, own(idx->st.thr_used, B * sizeof(float)));
    HIPCHECK(idx, idx->spec_moments.grow(B * kSpecSlabsMax * 2 * sizeof(float)));
    HIPCHECK(idx, idx->qdev.grow(B * idx->dim * sizeof(float)));
    HIPCHECK(idx, idx->cand_row.grow(B * kCandCapWide * sizeof(int32_t)));
    HIPCHECK(idx, idx->cand_val.grow(B * kCandCapWide * sizeof(float)));
    HIPCHECK(idx, idx->qlist_dev.grow(2 * B * sizeof(int)));  // second half: overflow re-runs
    HIPCHECK(idx, idx->status_host.grow((B + 1) * sizeof(int)));
    HIPCHECK(idx, idx->out_dist_dev.grow(B * kKMax * sizeof(double)));
    HIPCHECK(idx, idx->out_rows_dev.grow(B * kKMax * sizeof(int64_t)));
    HIPCHECK(idx, idx->out_count_dev.grow(B * sizeof(int64_t)));
    HIPCHECK(idx, idx->prune_skip.grow((2 + 2 * B) * sizeof(int)));
    HIPCHECK(idx, idx->stat_dev.grow(2 * B * sizeof(unsigned long long)));
    HIPCHECK(idx, hipMemsetAsync(idx->stat_dev, 0, 2 * B * sizeof(unsigned long long), idx->stream));
    // the prune / scan kernels use more than the default 64 KiB of dynamic LDS
    if (prune_lds_bytes(idx->dim, kPruneBigThreads, kPruneBigSort, 0) > 160 * 1024 || scan_lds_bytes(idx->dim, 1) > 160 * 1024)
        return fail(idx, MI355DR_E_UNSUPPORTED, "dim too large for the select kernels' LDS budget");
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_prune<kPruneBigThreads, kPruneBigSort>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)prune_lds_bytes(idx->dim, kPruneBigThreads, kPruneBigSort, 0)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_prune<kPruneSmallThreads, kPruneSmallSort>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)prune_lds_bytes(idx->dim, kPruneSmallThreads, kPruneSmallSort, idx->dpad)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_prune_wide<2, 32>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)prune_wide_lds_bytes(idx->dim, 2)));
    {
        int per = kScanQ;
        while (per > 1 && scan_lds_bytes(idx->dim, per) > 150 * 1024) per >>= 1;
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_scan, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)scan_lds_bytes(idx->dim, per)));
    }
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_scan32, hipFuncAttributeMaxDynamicSharedMemorySize, kScan32Lds));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_scan_ids, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)scan_ids_lds_bytes(idx->dim, kScanQ)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kScreenLds));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kScreenLds));
    {
        const int stream_lds = kStreamQueryBytesMax + kStreamStages * kStreamStageBytes;
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen_stream<false, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, stream_lds));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen_stream<true, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, stream_lds));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen_stream<false, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, stream_lds));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen_stream<true, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, stream_lds));
    }
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen256c<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kScreen256Lds));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen256c<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kScreen256Lds));
#define MI355_RQ_ATTR(KS)                                                                                              \
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen_rq<KS, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, rq_lds(KS)));
    MI355_RQ_FORMS(MI355_RQ_ATTR)
#undef MI355_RQ_ATTR
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_screen_rq<6, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, rq_lds(6)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_merge_topk, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kSortMax * 12));
    if (mmr_lds_bytes(idx->dim, kMmrMax) > 160 * 1024)
        return fail(idx, MI355DR_E_UNSUPPORTED, "dim too large for the select kernels' LDS budget");
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_mmr_select, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)mmr_lds_bytes(idx->dim, kMmrMax)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_shard_mmr_select, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)mmr_lds_bytes(idx->dim, kMmrMax)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_merge_groups, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)groups_lds_bytes(kSortMax)));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_collapse_lists, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)collapse_lds_bytes(kSortMax)));
    idx->qstate_ready = true;  // (behind the last step that can fail)
    return MI355DR_OK;
}

// bf16 screen bound E(d): |t - exact cosine key| <= 2^-7 + 2^-15 + 8*d*2^-24   (DESIGN.md "Screen bounds").
// bf16 keeps 8 significand bits: round-to-nearest has unit roundoff 2^-8 PER OPERAND, so a product of two rounded
// operands is off by up to 2^-7 + 2^-16 (relative), and by Cauchy-Schwarz so is the dot product of unit vectors.
inline float screen_bound(int d) {
    return (float)(std::ldexp(1.0, -7) + std::ldexp(1.0, -15) + 8.0 * d * std::ldexp(1.0, -24));
}

EventPair take_events(mi355dr_index* idx) {
    if (!idx->ev_pool.v.empty()) {
        EventPair p = idx->ev_pool.v.back();
        idx->ev_pool.v.pop_back();
        return p;
    }
    EventPair p{};
    (void)hipEventCreate(&p.a);
    (void)hipEventCreate(&p.b);
    return p;
}

void drain_events(mi355dr_index* idx) {  // the pairs whose launch has finished (a later block's may still be in flight)
    std::vector<EventPair> keep;
    for (auto& p : idx->ev_pending.v) {
        if (hipEventQuery(p.b) == hipErrorNotReady) {
            keep.push_back(p);
            continue;
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            idx->s_screen_ns += (int64_t)(ms * 1e6);
            if (p.big) idx->s_big_ns += (int64_t)(ms * 1e6);
        }
        idx->ev_pool.v.push_back(p);
    }
    idx->ev_pending.v.swap(keep);
}

// Candidates a chunk appends per query ~ k * (chunk / rows seen before) * inflation, where the inflation is how much
// the screen's bound widens the tail it has to keep: measured ~4-5 for the bf16 bound and ~14-16 for the int8 bound on
// Gaussian data.  The chunk growth is capped so that this stays inside what one prune of the one-wave kernel holds.
constexpr double kInflationBf16 = 5.0, kInflationI8 = 16.0;
constexpr double kSmallBlockBudget = 1.6;  // (the measured inflations are ~4 and ~9-10: the budget above carries that much slack)
// Round 6: passes at 33 <= k <= 128 prune with the two-wave form (k_prune_wide.h).  Its 4096 entries hold a chunk's appends
// AND the survivors carried from the chunk before; the first chunk behind the starter screens its rows from row 0, so it
// appends ~ k * inflation * ratio.  The inflation of the int8 bound at these k: 5.5 (k-th best of 64 k rows) ... 9.6 (of 10 M)
// by the Gaussian tail ratio, ~6 measured over the round-5 pass at k = 100 -- budgeted as 10 with a quarter of the entries spare.
constexpr double kInflationI8Wide = 10.0, kInflationBf16Wide = 4.0;
inline bool wide_ok(const mi355dr_index* idx, int k) { return idx->prune_wide && k >= kWideKMin && k <= kWideKMax; }
inline double growth_budget(const mi355dr_index* idx, int k, bool i8) {
    if (wide_ok(idx, k) && idx->path != MI355DR_PATH_SCAN) {
        const int room = std::min(kWideEntries, idx->cap_set ? idx->cap : kCandCapWide);
        return 0.75 * room / ((double)k * (i8 ? idx->wide_inflation_x10 / 10.0 : kInflationBf16Wide)) - 1.0;  // (1 + growth = the chunk ratio)
    }
    const int room = k < kPruneSmallSort / 2 ? kPruneSmallSort - k : idx->cap;  // (large k: the general prune, whole buffer)
    return 0.6 * std::min(room, idx->cap) / ((double)k * (i8 ? kInflationI8 : kInflationBf16));
}

// THE decision of a pass at k and fix-up level `level` (force_scan: as under path = scan, whatever the option says), made once
// from the handle's options and corpus as they are now and handed down as a value.  `no_screen`: the caller's text for a
// path = screen pass that no screen can serve (the int8 refusal reads the same everywhere).
// Which screen: int8 needs a corpus that quantised within the limit and (in AUTO) a k small enough that its wider bound still
// allows chunks to grow (k <= 133 at the default budget line); larger k keeps bf16.
inline bool i8_available(const mi355dr_index* idx) { return idx->irr8_n <= kIrrCap; }
constexpr int kStarterKMax = 32;          // the starter's round A re-scores max(32, 2k) <= 64 rows: one batch of the one-wave form
constexpr int64_t kStarterRows = 16384;   // sample size (256 slabs); a corpus must hold at least 4 samples
static_assert(kStarterRows / kSlabRows <= kSpecSlabsMax, "the moment scratch holds one entry per slab of the starter's sample");
// rows the starter of a pass samples, 0 if the pass takes the emit-all ladder (the reasons: plan_pass)
int64_t starter_sample_rows(const mi355dr_index* idx, const Pass& ps) {
    const int64_t n = idx->n;
    const int64_t rows = std::min<int64_t>(ps.wide ? idx->starter_rows_wide : kStarterRows, n / 4) / kTileM * kTileM;
    const int64_t slabs = (rows + kSlabRows - 1) / kSlabRows;
    const bool take = idx->starter && (ps.k <= kStarterKMax || ps.wide) && ps.level == 0 && idx->chunk0_set == 0 && n >= 4 * 1024 &&
                      slabs <= ps.cap && slabs >= ps.k;
    return take ? rows : 0;
}
Pass decide_pass(const mi355dr_index* idx, int k, int level, bool force_scan, const char* no_screen = nullptr) {
    Pass ps;
    ps.k = k;
    ps.level = level;
    const int path = force_scan ? (int)MI355DR_PATH_SCAN : idx->path;
    if (level > 0) ps.i8 = false;  // re-screening overflowed queries: the ~3x tighter bf16 bound
    else if (idx->screen_dtype == MI355DR_SCREEN_I8) ps.i8 = true;
    // (measured round 3, N = 10 M, 1024 queries: int8 7.4 / 8.0 / 9.5 / 11.7 / 12.7 ms at k = 10 / 32 / 64 / 100 / 128 against
    // 13-14.4 ms for bf16, whose kernel alone is 11 ms; 22 against 16 at k = 200, where the int8 chunks hardly grow any more:
    // the cross-over is near k = 160, budget 0.2; round 2 drew the line at k = 24, budget 1.5)
    else ps.i8 = idx->screen_dtype == MI355DR_SCREEN_AUTO && i8_available(idx) && k < idx->i8_demoted_k &&
                 growth_budget(idx, k, true) >= idx->i8_min_budget;
    // (inner product rides the same cosine screens: thresholds become cos >= dot_k / (|q| cmax), see k_prune)
    const bool screen_possible = ps.i8 ? i8_available(idx) : idx->irr_n <= kIrrCap;
    ps.screening = idx->n > 0 && screen_possible && path != MI355DR_PATH_SCAN;
    // the two-wave prune and its 4096-slot lists are for passes that screen: the exact scan keeps the general form and its
    // <= 2048-slot lists, on path = scan and on an AUTO pass no screen can serve alike
    ps.wide = ps.screening && wide_ok(idx, k);
    ps.cap = !idx->cap_set && ps.wide ? kCandCapWide : idx->cap;
    if (idx->screen_dtype == MI355DR_SCREEN_I8 && !i8_available(idx) && path != MI355DR_PATH_SCAN)
        ps.refused = "int8 screen unavailable: too many rows outside the residual limit";
    else if (path == MI355DR_PATH_SCREEN && !screen_possible && idx->n > 0) ps.refused = no_screen;
    // speculative one-chunk pass: m(k) inside the one-wave prune's budget (the compiled-in table holds only such k: the
    // inequality is tools/spec_model.py's, checked again here for a list stride the caller shrank)
    ps.spec_m = spec_m_of(k);
    // (spec_eligible: everything but the probation -- enqueue_block counts a suspension down on exactly these passes)
    ps.spec_eligible = level == 0 && ps.screening && !ps.wide && ps.spec_m > 0 && idx->speculate && idx->n >= idx->spec_min_rows &&
                       kSpecInflation * ps.spec_m * 4 <= 3 * (std::min(kPruneSmallSort, ps.cap) - k) &&
                       starter_sample_rows(idx, ps) > 0;
    ps.speculative = ps.spec_eligible && idx->spec_probation <= 0;
    return ps;
}
// between searches (stat "screen_dtype_active", the debug entry points): the screen a first attempt at the last k would take
inline bool idle_i8(const mi355dr_index* idx) { return decide_pass(idx, idx->last_pass_k, 0, false).i8; }

int launch_prune(mi355dr_index* idx, hipStream_t s, const Pass& ps, int nblocks, const int* qlist, int exact,
                 bool thr_only = false, bool one_wave_only = false, bool defer_b = false, const SpecModel* spec = nullptr) {
    PruneArgs pa{};
    if (spec) pa.spec = *spec;  // (the starter's prune of a speculative pass)
    pa.thr_only = thr_only ? 1 : 0;
    pa.one_wave_only = one_wave_only ? 1 : 0;
    pa.defer_b = defer_b && idx->defer_round_b ? 1 : 0;
    pa.rows = idx->rows;
    pa.nrm2 = idx->nrm2;
    pa.q = idx->qdev;
    pa.st = idx->st;
    pa.cand_row = idx->cand_row;
    pa.cand_val = idx->cand_val;
    pa.qlist = qlist;
    pa.stat = idx->stat_dev;
    pa.cap = ps.cap;
    pa.d = idx->dim;
    pa.k = ps.k;
    pa.metric = idx->metric;
    pa.exact = exact;
    // (flags exist only for loose rows, and every loose row is counted: a corpus without any -- the usual case -- spares each
    // candidate the dependent flag8[row] load, one memory round trip of the prune's latency chain)
    // (a removed row carries the flag too -- its all-zero int8 image can pass a low threshold -- and is in no list: dead_n)
    pa.flag8 = (ps.i8 && (idx->irr8_n > 0 || idx->dead_n > 0)) ? idx->flag8 : nullptr;
    pa.cscale = idx->metric == MI355DR_METRIC_IP ? idx->cmax : 1.0f;
    // int8 screen, cosine: candidates that survive the exact cut are screened once more on their bf16 shadow rows
    // (half the bytes of an fp32 row, a bound ~5x tighter) before the exact re-score
    pa.shadow16 = (ps.i8 && idx->metric == 0 && !exact && idx->prefilter16) ? idx->shadow : nullptr;
    pa.dpad = idx->dpad;
    pa.round_a = idx->round_a;
    // the general form walks the (usually empty) list of queries the one-wave form left, on a small grid
    if (!exact && ps.wide) {  // 33 <= k <= 128: the two-wave form alone (what it cannot hold is flagged for the re-screen)
        pa.shadow16 = nullptr;
        hipLaunchKernelGGL((k_prune_wide<2, 32>), dim3(nblocks), dim3(2 * kWave), prune_wide_lds_bytes(idx->dim, 2), s, pa);
        HIPCHECK(idx, hipGetLastError());
        return MI355DR_OK;
    }
    // (its sort holds k kept entries and one whole list: kSortMax >= kKMax + kCandCap, dev_common.h)
    if (pa.cap > kCandCap) return fail(idx, MI355DR_E_INTERNAL, "general-form prune on a list stride above kCandCap");
    const bool list_mode = qlist == nullptr;
    pa.skip_list = list_mode ? idx->prune_skip : nullptr;
    pa.skip_parity = list_mode ? (idx->prune_parity ^= 1) : 0;
    // small instantiation first (common case, whole block resident), then the large one for what it skipped
    hipLaunchKernelGGL((k_prune<kPruneSmallThreads, kPruneSmallSort>), dim3(nblocks), dim3(kPruneSmallThreads),
                       prune_lds_bytes(idx->dim, kPruneSmallThreads, kPruneSmallSort, pa.shadow16 ? idx->dpad : 0), s, pa);
    HIPCHECK(idx, hipGetLastError());
    if (one_wave_only) return MI355DR_OK;  // (what the one-wave form cannot hold is flagged for the host's re-screen)
    hipLaunchKernelGGL((k_prune<kPruneBigThreads, kPruneBigSort>), dim3(list_mode ? std::min(nblocks, 64) : nblocks),
                       dim3(kPruneBigThreads), prune_lds_bytes(idx->dim, kPruneBigThreads, kPruneBigSort, 0), s, pa);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

int launch_prep(mi355dr_index* idx, hipStream_t s, int B, int Bpad, int metric, bool i8, int cnt0 = 0) {
    hipLaunchKernelGGL(k_prep_queries, dim3(Bpad), dim3(64), (size_t)idx->dim * sizeof(float), s, idx->qdev, B, idx->dim,
                       idx->dpad, metric, idx->st, idx->dpad8, i8 ? 1 : 0, idx->bf16_ec, idx->status_or_dev,
                       idx->prune_skip, cnt0, idx->metric == MI355DR_METRIC_IP ? idx->cmax : 1.0f);
    idx->prune_parity = 0;
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// tile edge used for a block of B queries: the 256x256 ping-pong kernel from 129 queries up, else 128x128
inline int screen_tile(int B) { return B > kTileN ? kT2 : kTileM; }

constexpr int kRetryLevels = 2;  // re-screens of an overflowed query (bf16, growth/2, then growth 0.25) before the exact scan

// which kernel one screen launch over `rows` rows takes (launch_screen switches on it; mi355dr_debug_screen_hits reports it)
enum ScreenKernel { kKernTile = 0, kKernStream = 1, kKern256c = 2, kKernRq = 3 };
inline ScreenKernel screen_kernel_for(const mi355dr_index* idx, bool i8, int B, int64_t rows, bool emit_all) {
    // the emit-all first chunk always goes through the 128x128 kernel (k_screen256c and k_screen_rq have no emit-all epilogue)
    // ... and so do chunks of a few thousand rows: their thresholds are still so low that a good part of the tile is a
    // hit, which the per-lane global append of k_screen handles better than the small per-wave queues of k_screen256c and k_screen_rq
    const int tile = (emit_all || rows <= idx->small_chunk_rows) ? kTileM : screen_tile(B);
    const int row_bytes = i8 ? idx->dpad8 : idx->dpad * 2;
    const int ksteps = row_bytes / kRowB;
    // query operand resident in registers, 128-row tiles (k_screen_rq.h): int8 shadows of at most 768 bytes per row
    if (tile == kT2) return i8 && idx->screen_rq && screen_rq_has(ksteps) ? kKernRq : kKern256c;
    // small query blocks: the streaming form (resident query block, deep row ring, one persistent workgroup per CU)
    if (!emit_all && idx->screen_stream && B <= 64 && ksteps >= 1 && (B <= 32 ? 32 : 64) * row_bytes <= kStreamQueryBytesMax)
        return kKernStream;
    return kKernTile;
}

// launch one screen pass over rows [r0, r_end) (r0 a multiple of the tile edge); flush_mask: k_screen_rq's common flush
// period - 1 (-1: every wave on its own)
int launch_screen(mi355dr_index* idx, hipStream_t s, bool i8, int B, int64_t r0, int64_t r_end, int cap, int emit_mode,
                  int flush_mask, int moment_slabs = 0) {
    const bool emit_all = emit_mode != 0;  // (both special epilogues live in k_screen)
    const ScreenKernel kern = screen_kernel_for(idx, i8, B, r_end - r0, emit_all);
    const int tile = kern == kKern256c || kern == kKernRq ? kT2 : kTileM;
    ScreenArgs2 sa{};
    sa.status = idx->st.status;
    sa.shadow = i8 ? (const void*)idx->shadow8 : (const void*)idx->shadow;
    sa.qhat = i8 ? (const void*)idx->st.qhat8 : (const void*)idx->st.qhat;
    sa.thr = idx->st.thr;
    sa.sc = idx->st.sc;
    sa.kq = idx->st.kq;
    sa.grp = idx->grp8;
    sa.flag8 = idx->flag8;
    sa.cnt = idx->st.cnt;
    sa.cand_row = idx->cand_row;
    sa.cand_val = idx->cand_val;
    sa.row_bytes = i8 ? idx->dpad8 : idx->dpad * 2;
    sa.ksteps = sa.row_bytes / kRowB;
    sa.cap = cap;
    sa.ct0 = (int)(r0 / tile);
    sa.n_ctiles = (int)(round_up(r_end, tile) / tile) - sa.ct0;
    sa.n_qtiles = (int)(round_up(B, tile) / tile);
    sa.row_end = r_end;
    sa.row0 = r0;
    sa.emit_all = emit_mode;
    if (moment_slabs > 0) {  // the starter of a speculative pass: per-slab sums behind the slab maxima
        sa.moments = idx->spec_moments;
        sa.moment_slabs = moment_slabs;
    }
    const int64_t grid = round_up(sa.n_ctiles, 8) * sa.n_qtiles;
    switch (kern) {
    case kKernRq: {
        sa.ct0 = (int)(r0 / kRqRows);
        sa.n_ctiles = (int)(round_up(r_end, kRqRows) / kRqRows) - sa.ct0;
        const unsigned g2 = screen_rq_grid(sa.n_ctiles, sa.n_qtiles);
        idx->s_rq_launches++;
        if (idx->debug_park > 0 && r_end - r0 >= idx->debug_park) {  // (diagnostic: thresholds at +inf for a launch of at least that many rows -- its cost without a single hit; results are WRONG)
            if (!idx->park_thr) {
                std::vector<float> inf(kQBlockMax, INFINITY);
                HIPCHECK(idx, idx->park_thr.grow(kQBlockMax * sizeof(float)));
                HIPCHECK(idx, hipMemcpy(idx->park_thr, inf.data(), kQBlockMax * sizeof(float), hipMemcpyHostToDevice));
            }
            sa.thr = idx->park_thr;
        }
        sa.progress = idx->rq_progress;  // sibling drift limiter: words of older launches carry another stamp and are ignored
        sa.epoch = idx->rq_epoch = idx->rq_epoch % 4095 + 1;
        // (the stamp has 12 bits: when it wraps, words left by launches 4095 stamps ago are cleared so that none of them can
        // pass for a sibling of this launch -- a stale word could only cost a capped wait, never a result)
        if (sa.epoch == 1) HIPCHECK(idx, hipMemsetAsync(idx->rq_progress, 0, kRqProgressWords * sizeof(int), s));
        sa.drift = idx->screen_drift;
        sa.flush_mask = flush_mask;
        sa.flush_alone = idx->screen_flush_alone;
        if (sa.ksteps == 6 && !idx->screen_rq_split_tests) {  // (A/B form, d = 768 only: every block test in one piece)
            hipLaunchKernelGGL((k_screen_rq<6, false, true>), dim3(g2), dim3(512), rq_lds(6), s, sa);
        } else {
            switch (sa.ksteps) {
#define MI355_RQ_LAUNCH(KS) \
    case KS: hipLaunchKernelGGL((k_screen_rq<KS, true, true>), dim3(g2), dim3(512), rq_lds(KS), s, sa); break;
                MI355_RQ_FORMS(MI355_RQ_LAUNCH)
#undef MI355_RQ_LAUNCH
            }
        }
        break;
    }
    case kKern256c: {
        const unsigned g2 = screen256_grid(sa.n_ctiles, sa.n_qtiles);  // persistent: <= one workgroup per CU
        if (i8) hipLaunchKernelGGL((k_screen256c<true>), dim3(g2), dim3(512), kScreen256Lds, s, sa);
        else hipLaunchKernelGGL((k_screen256c<false>), dim3(g2), dim3(512), kScreen256Lds, s, sa);
        break;
    }
    case kKernStream: {
        const int nq = B <= 32 ? 32 : 64;
        const unsigned gs = (unsigned)std::min(sa.n_ctiles, 256);
        const size_t lds = screen_stream_lds(nq, sa.row_bytes);
        if (i8 && nq == 32) hipLaunchKernelGGL((k_screen_stream<true, 32>), dim3(gs), dim3(256), lds, s, (ScreenArgs)sa);
        else if (i8) hipLaunchKernelGGL((k_screen_stream<true, 64>), dim3(gs), dim3(256), lds, s, (ScreenArgs)sa);
        else if (nq == 32) hipLaunchKernelGGL((k_screen_stream<false, 32>), dim3(gs), dim3(256), lds, s, (ScreenArgs)sa);
        else hipLaunchKernelGGL((k_screen_stream<false, 64>), dim3(gs), dim3(256), lds, s, (ScreenArgs)sa);
        break;
    }
    case kKernTile:
        if (i8) hipLaunchKernelGGL(k_screen<true>, dim3((unsigned)grid), dim3(256), kScreenLds, s, (ScreenArgs)sa);
        else hipLaunchKernelGGL(k_screen<false>, dim3((unsigned)grid), dim3(256), kScreenLds, s, (ScreenArgs)sa);
        break;
    }
    HIPCHECK(idx, hipGetLastError());
    if (emit_mode == kEmitAll) {  // every row of the chunk was stored at slot row-r0 for every query
        // (the starter's one-candidate-per-slab count is what k_prep_queries initialised the lists with: starter_count())
        const int per_query = (int)(r_end - r0);
        hipLaunchKernelGGL(k_set_counts, dim3((B + 255) / 256), dim3(256), 0, s, idx->st.cnt, B, per_query);
        HIPCHECK(idx, hipGetLastError());
    }
    return MI355DR_OK;
}

// ---- the pass schedule --------------------------------------------------------------------------------------------
// Thresholds are frozen during a launch, so the corpus is walked in geometrically growing chunks, each followed by the exact
// re-score + select of what it appended (k_prune), which publishes the next chunk's thresholds.  Round 3:
//  * STARTER instead of the three smallest chunks (k <= kStarterKMax, first attempt only): one k_screen launch over the first
//    S <= 16 k rows that keeps, per query, the best value of every 64-row slab (S / 64 candidates, no thresholds, no atomics)
//    + one k_prune (thr_only) that re-scores the best-looking of them exactly and publishes the threshold their k-th best
//    gives -- valid whatever the sample missed -- and keeps nothing; the first regular chunk then starts at row 0.  Two
//    launches (~80 us) where the ladder 1 024 -> 4 096 -> 16 384 took six (~290 us), at every shard size.
//  * The chunk ends are PLANNED: n = the fewest steps of ratio <= 1 + growth from the starter's sample (or the emit-all first
//    chunk) to the end, then one uniform ratio (N / S)^(1/n) -- no short last chunk with a prune of its own.
//  * (Option prune_companion = 0: no general-form launch behind the one-wave prune, what it cannot hold is flagged and
//    re-screened -- measured slower: see index.h.)
// (kStarterKMax, kStarterRows: above decide_pass; a pass at 33 <= k <= 128 samples idx->starter_rows_wide rows: 65536 = 1024 slabs
// by default)
//  * SPECULATIVE passes (Pass::speculative): the starter, then ONE chunk over all rows at the threshold the
//    starter's prune predicts from the sample's moments; k_finalize verifies it, complete_block re-runs what it rejects.
struct PassPlan {
    int64_t sample = 0;          // > 0: starter over rows [0, sample)
    std::vector<int64_t> ends;   // chunk ends, ascending, last = n; the first chunk starts at 0 (starter) or is the emit-all one
    bool emit_all_first = false;
};
PassPlan plan_pass(const mi355dr_index* idx, const Pass& ps, int B, double growth) {
    PassPlan p;
    const int64_t n = idx->n;
    const int cap = ps.cap;
    const bool wide = ps.wide;
    const int tile = screen_tile(B);
    int64_t seen = 0;  // rows whose k-th best the first planned chunk's threshold comes from
    // the starter leaves one candidate per 64-row slab of its sample in every query's list: the list must hold them
    // (option cand_cap goes down to 16: with fewer slots than slabs every list would start past its end and the whole block
    // would be flagged for a re-screen), and the sample must offer at least k of them, else its prune publishes no threshold
    // and the first regular chunk would run at thr = -inf WITHOUT the emit-all epilogue -- correct, pathologically slow
    // (4096 <= n < 8192 with k in 17..32).  Either way: the emit-all ladder.
    // Round 6, 33 <= k <= 128 (two-wave prune): the same estimator over a 64 k-row sample -- 1024 slab maxima per query, of
    // which the prune re-scores the 128 best-looking; their k-th best exact score is (about) the k-th best of the sample.
    const int64_t starter_rows = starter_sample_rows(idx, ps);
    if (starter_rows > 0) {
        p.sample = starter_rows;
        seen = p.sample;
        if (ps.speculative) {  // one chunk: its threshold does not come from rows seen before
            p.ends.push_back(n);
            return p;
        }
    } else {
        const int64_t c0 = std::min<int64_t>(n, round_up(std::max<int64_t>(tile, std::min<int64_t>(idx->chunk0_rows, cap)), tile));
        p.emit_all_first = c0 <= cap;
        p.ends.push_back(c0);
        seen = c0;
        if (c0 >= n) return p;
    }
    const double rmax = 1.0 + growth;
    const double span = (double)n / (double)seen;
    // (0.15: a span a hair above a power of the ratio -- 1.25 M rows behind a 16 k sample, the 8-way shard of the headline corpus --
    // takes the smaller number of chunks: 3 instead of 4 there, 1.136 against 1.156 ms per pass with k_screen_rq, whose hits cost
    // less than a chunk boundary; 5 M rows take 4 instead of 5: 3.50 against 3.49 ms; profiles/r05_chunk_sweep.txt)
    int steps = std::max(1, (int)std::ceil(std::log(span) / std::log(rmax) - 0.15));
    const double r = std::pow(span, 1.0 / steps);
    // tapered ratios (same product): r_i = r * t^((steps-1)/2 - i); the first (largest) one stays within what the lists hold
    double taper = std::max(1.0, (idx->chunk_taper_x100 > 0 ? idx->chunk_taper_x100 : (wide ? 120 : 100)) / 100.0);
    if (steps > 1 && taper > 1.0) {
        const double room = std::max(1.0, rmax * 1.25 / r);  // (the budget line already keeps a quarter / 40 % of the entries spare)
        taper = std::min(taper, std::pow(room, 2.0 / (steps - 1)));
    } else {
        taper = 1.0;
    }
    double pos = (double)seen;
    int64_t prev = p.sample > 0 ? 0 : seen;
    for (int i = 1; i <= steps; ++i) {
        pos *= r * std::pow(taper, (steps - 1) / 2.0 - (i - 1));
        int64_t end = i == steps ? n : std::min<int64_t>(n, round_up((int64_t)pos, tile));
        if (tile == kT2 && end < n) {
            // whole rounds of the persistent grid: 8 XCDs x (32 / n_qtiles) corpus tiles are in flight at a time, and a chunk
            // of 4.3 rounds costs 5 (k_screen256c's launches of 70 k rows ran at 1.6 ns per row against 0.68 in long ones)
            const int n_qtiles = (int)(round_up(B, kT2) / kT2);
            const int64_t round_rows = (int64_t)8 * (32 / n_qtiles) * kT2;
            const int64_t len = end - prev;
            if (len >= 2 * round_rows) end = std::min<int64_t>(n, prev + (len + round_rows / 2) / round_rows * round_rows);
        }
        if (end <= prev) continue;
        p.ends.push_back(end);
        prev = end;
        if (end >= n) break;
    }
    if (p.ends.empty() || p.ends.back() < n) p.ends.push_back(n);
    return p;
}

inline int starter_count(const PassPlan& p) { return (int)((p.sample + kSlabRows - 1) / kSlabRows); }

// Phi^-1(p), 0 < p < 1, by bisection on erfc (host, once per speculative pass; tools/spec_model.py does the same)
inline double normal_quantile(double p) {
    double lo = -40.0, hi = 40.0;
    for (int i = 0; i < 200; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (0.5 * std::erfc(-mid / std::sqrt(2.0)) < p) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// what the starter's prune of a speculative pass predicts from (run_screen; mi355dr_debug_spec_model).  zq = Phi^-1(1 - m / n):
// the Gaussian quantile above which m of the n rows are expected (no inverse error function on the device); the lab shift
// makes the model wrong on purpose.  n counts removed rows, and the sums run over the sample's rows, removed ones included
// (DESIGN.md 4.3 "On a mutated index").  *zq_out: the quantile before its rounding to float.
SpecModel spec_model(const mi355dr_index* idx, const Pass& ps, const PassPlan& plan, double* zq_out = nullptr) {
    SpecModel sm{};
    sm.moments = idx->spec_moments;
    sm.slabs = starter_count(plan);
    sm.rows = (int)plan.sample;
    const double zq = normal_quantile(1.0 - (double)ps.spec_m / (double)idx->n) + idx->spec_shift_milli / 1000.0;
    sm.zq = (float)zq;
    if (zq_out) *zq_out = zq;
    return sm;
}

PassPlan make_plan(const mi355dr_index* idx, const Pass& ps, int B) {
    // (measured round 3, N = 10 M, k = 10: a ratio of 4 per step -- 5 chunks -- 7.43 ms, the budget's 4.8 -- 4 chunks -- 7.54)
    const double budget = growth_budget(idx, ps.k, ps.i8);
    double growth = std::max(0.25, std::min((double)idx->chunk_growth, budget));
    // small query blocks: a pass is one stream over the shadow rows plus one latency-bound re-score launch per chunk, and an
    // append costs nothing -- fewer, larger chunks (the k-dependent budget alone bounds the growth: x7 per step at k = 10)
    if (B <= 64 && ps.level == 0 && idx->chunk_growth_set == 0) growth = std::max(growth, std::min(8.0, budget * kSmallBlockBudget));
    if (ps.level == 1) growth = std::max(0.25, growth * 0.5);
    if (ps.level >= 2) growth = 0.25;  // (every chunk then holds <= 20 % of the rows: a dense neighbourhood is split up)
    return plan_pass(idx, ps, B, growth);
}

// screen path over all rows for the B queries prepared in idx->st / idx->qdev (candidate counts initialised to
// starter_count(plan) by k_prep_queries when the plan has a starter)
int run_screen(mi355dr_index* idx, hipStream_t s, const Pass& ps, int B, const PassPlan& plan) {
    int64_t kept_all_below = 0;  // rows the emit-all first chunk already turned into candidates
    const bool i8 = ps.i8;
    const int side_n = i8 ? idx->irr8_n : idx->irr_n;  // rows this screen cannot see
    constexpr int kSideMerge = 32;
    bool side_done = false;
    // one-wave prune alone: small k, first attempt (a retry keeps the general form: it is the last screen before the exact scan)
    const bool lean = plan.sample > 0 && idx->prune_companion == 0;
    auto timed = [&](bool big, int64_t rows, auto&& launch) -> int {
        EventPair ev{};
        if (idx->profile) {
            ev = take_events(idx);
            HIPCHECK(idx, hipEventRecord(ev.a, s));
        }
        CHECK(launch());
        if (idx->profile) {
            HIPCHECK(idx, hipEventRecord(ev.b, s));
            ev.big = big ? 1 : 0;
            idx->ev_pending.v.push_back(ev);
        }
        idx->s_screen_launches++;
        idx->s_screen_rows += rows;
        if (big) {
            idx->s_big_launches++;
            idx->s_big_rows += rows;
        }
        return MI355DR_OK;
    };
    if (plan.sample > 0) {
        // (the flush mask: none of the slab-maximum epilogue's kernels reads it)
        SpecModel sm{};
        if (ps.speculative) {
            sm = spec_model(idx, ps, plan);
            idx->s_spec_passes++;
        }
        CHECK(timed(false, plan.sample, [&] {
            return launch_screen(idx, s, i8, B, 0, plan.sample, ps.cap, kEmitSlabMax, -1, ps.speculative ? sm.slabs : 0);
        }));
        CHECK(launch_prune(idx, s, ps, B, nullptr, /*exact=*/0, /*thr_only=*/true, /*one_wave_only=*/true, false,
                           ps.speculative ? &sm : nullptr));
        idx->s_starters++;
    }
    int64_t done = 0;
    for (size_t ci = 0; ci < plan.ends.size(); ++ci) {
        const int64_t end = plan.ends[ci];
        const bool emit_all = ci == 0 && plan.emit_all_first;
        if (emit_all) kept_all_below = end;
        // the first chunk has no threshold yet: it keeps every row (direct stores) as long as it fits the buffer
        const bool big = !emit_all && end - done > idx->small_chunk_rows && screen_tile(B) == kT2;
        // hit lanes a wave of k_screen_rq expects per tile (32 queries x 128 rows): rows above the threshold of `seen` rows
        // ~ k x inflation / seen per row and query (inflation of the int8 bound ~8)
        const int64_t seen = ci == 0 ? (plan.sample > 0 ? plan.sample : end) : done;
        // (a speculative pass's one chunk: kSpecInflation x m candidates expected over all n rows, whatever was seen before)
        const double lanes = ps.speculative ? (double)kSpecInflation * ps.spec_m * 4096.0 / (double)idx->n
                                            : 8.0 * ps.k * 4096.0 / (double)std::max<int64_t>(seen, 1);
        int period = 1;
        while (period < 64 && period * 2 * lanes <= idx->screen_flush_lanes) period *= 2;
        const int flush_mask = idx->screen_flush_sync ? period - 1 : -1;
        CHECK(timed(big, end - done, [&] { return launch_screen(idx, s, i8, B, done, end, ps.cap, emit_all ? kEmitAll : 0, flush_mask); }));
        idx->s_chunks++;
        if (end >= idx->n && side_n > 0 && side_n <= kSideMerge) {
            // rows this screen cannot see (irregular; for int8 also loose): a handful of them ride the LAST chunk's prune
            // as "no bound" candidates instead of costing a prune pass of their own (0.12 ms per block at N = 10 M)
            hipLaunchKernelGGL(k_emit_irregular, dim3(B), dim3(64), 0, s, i8 ? idx->irr8_rows : idx->irr_rows, side_n, idx->st,
                               idx->cand_row, idx->cand_val, ps.cap, (int)kept_all_below);
            HIPCHECK(idx, hipGetLastError());
            side_done = true;
        }
        // every prune but the pass's last one carries its survivors over instead of re-scoring them (k_prune: defer_b)
        const bool last = end >= idx->n && (side_n == 0 || side_done);
        CHECK(launch_prune(idx, s, ps, B, nullptr, /*exact=*/0, false, lean, !last));
        done = end;
    }
    if (side_n > 0 && !side_done) {
        hipLaunchKernelGGL(k_emit_irregular, dim3(B), dim3(64), 0, s, i8 ? idx->irr8_rows : idx->irr_rows, side_n, idx->st,
                           idx->cand_row, idx->cand_val, ps.cap, (int)kept_all_below);
        HIPCHECK(idx, hipGetLastError());
        CHECK(launch_prune(idx, s, ps, B, nullptr, 0, false, lean));
    }
    idx->s_passes++;
    return MI355DR_OK;
}

// one exact-scan launch over rows [r0, r1) for the nq <= kScanQ queries of `qlist` (device memory).  ids != nullptr: the gathered
// scan (mi355dr_search_subset) over list POSITIONS [r0, r1) of those local rows
int launch_scan(mi355dr_index* idx, hipStream_t s, const int* qlist, int nq, int cap, int64_t r0, int64_t r1,
                const int32_t* ids = nullptr) {
    ScanArgs sa{};
    sa.rows = idx->rows;
    sa.nrm2 = idx->nrm2;
    sa.q = idx->qdev;
    sa.st = idx->st;
    sa.cand_row = idx->cand_row;
    sa.cand_val = idx->cand_val;
    sa.qlist = qlist;
    sa.nq = nq;
    sa.cap = cap;
    sa.d = idx->dim;
    sa.metric = idx->metric;
    sa.row0 = r0;
    sa.row1 = r1;
    const dim3 grid((unsigned)((r1 - r0 + kScanThreads - 1) / kScanThreads));
    const ScanIdsArgs ia{sa, ids};
    if (ids) hipLaunchKernelGGL(k_scan_ids, grid, dim3(kScanThreads), scan_ids_lds_bytes(idx->dim, nq), s, ia);
    else if (idx->dim % kScan32PieceCols == 0 && idx->scan_dma)  // rows are whole 128-byte pieces: the LDS-DMA form
        hipLaunchKernelGGL(k_scan32, grid, dim3(kScanThreads), kScan32Lds, s, sa, idx->n);
    else hipLaunchKernelGGL(k_scan, grid, dim3(kScanThreads), scan_lds_bytes(idx->dim, nq), s, sa);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// that launch for the queries in qlist_dev[off..off+nq), then their exact prune
int scan_range(mi355dr_index* idx, hipStream_t s, const Pass& ps, int off, int nq, int64_t r0, int64_t r1, const int32_t* ids) {
    CHECK(launch_scan(idx, s, idx->qlist_dev + off, nq, ps.cap, r0, r1, ids));
    return launch_prune(idx, s, ps, nq, idx->qlist_dev + off, /*exact=*/1);
}

// guaranteed exact path for the queries listed in `qs` (indices into the current block) over the index's `total` rows, or
// (ids != nullptr) over the `total` positions of a sorted id list -- positions are in row order, and a sorted corpus is as
// adversarial there as here.  The plain form returns without a synchronisation unless a chunk overflowed (asynchronous
// blocks rely on that); the gathered form is complete on return.
int run_scan(mi355dr_index* idx, hipStream_t s, const Pass& ps, const std::vector<int>& qs, int64_t total,
             const int32_t* ids = nullptr) {
    if (qs.empty()) return MI355DR_OK;
    HIPCHECK(idx, hipMemcpyAsync(idx->qlist_dev, qs.data(), qs.size() * sizeof(int), hipMemcpyHostToDevice, s));
    const int nq_all = (int)qs.size(), cap = ps.cap;
    hipLaunchKernelGGL(k_reset_queries, dim3((nq_all + 255) / 256), dim3(256), 0, s, idx->st, idx->qlist_dev, nq_all);
    HIPCHECK(idx, hipGetLastError());
    const int per = kScanQ;  // queries per launch: one 32-column MFMA block (LDS use does not depend on the dimension)
    for (int off = 0; off < nq_all; off += per) {
        const int nq = std::min(per, nq_all - off);
        int64_t done = 0;
        int64_t chunk = std::min<int64_t>(idx->chunk0_rows, cap);
        while (done < total) {
            const int64_t end = std::min<int64_t>(total, done + chunk);
            CHECK(scan_range(idx, s, ps, off, nq, done, end, ids));
            if (end - done > cap) {  // only a chunk larger than the buffer can overflow
                HIPCHECK(idx, hipMemcpyAsync(idx->status_host, idx->st.status, kQBlockMax * sizeof(int),
                                             hipMemcpyDeviceToHost, s));
                HIPCHECK(idx, hipStreamSynchronize(s));
                std::vector<int> redo;
                for (int j = 0; j < nq; ++j)
                    if (idx->status_host[qs[off + j]] & kStOverflow) redo.push_back(qs[off + j]);
                if (!redo.empty()) {
                    // re-run this range for the overflowed queries in buffer-sized pieces (cannot overflow);
                    // the other queries of the group already committed it.  Uses the tail of qlist_dev.
                    const int roff = kQBlockMax;
                    HIPCHECK(idx, hipMemcpyAsync(idx->qlist_dev + roff, redo.data(), redo.size() * sizeof(int),
                                                 hipMemcpyHostToDevice, s));
                    // clear the overflow bit but keep the kept list (prune did not commit the failed chunk)
                    for (int q : redo) idx->status_host[q] &= ~kStOverflow;
                    for (int q : redo)
                        HIPCHECK(idx, hipMemcpyAsync(idx->st.status + q, idx->status_host + q, sizeof(int),
                                                     hipMemcpyHostToDevice, s));
                    for (int64_t p = done; p < end; p += cap)
                        CHECK(scan_range(idx, s, ps, roff, (int)redo.size(), p, std::min<int64_t>(end, p + cap), ids));
                    if (ids) {
                        HIPCHECK(idx, hipStreamSynchronize(s));  // `redo` (pageable) was read by the copy
                        idx->s_subset_rerun_queries += (int64_t)redo.size();
                    }
                }
            }
            done = end;
            // exact keys: a chunk only appends the rows that enter the running top-k (k ln(ratio) of them on unordered data),
            // so the ladder can be steep (x64) -- 3 launches and prunes for 2 M rows instead of 7 (an adversarial order overflows
            // the list and takes the buffer-sized re-run above)
            chunk = std::max<int64_t>(chunk, done * (idx->chunk_growth_set ? idx->chunk_growth : 63));
        }
    }
    if (ids) HIPCHECK(idx, hipStreamSynchronize(s));  // `qs` (pageable) was read by the copy
    else idx->s_fallback_queries += nq_all;
    return MI355DR_OK;
}

// one block of B <= kQBlockMax device-resident queries against the m uploaded ids -> device outputs [B,k], complete on return
int subset_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int B, int k, int64_t m, double* out_dist_dev,
                 int64_t* out_rows_dev) {
    const Pass ps = decide_pass(idx, k, 0, /*force_scan=*/true);  // (it never screens: the exact path's list stride)
    idx->last_pass_k = k;
    if (q_dev != idx->qdev)
        HIPCHECK(idx, hipMemcpyAsync(idx->qdev, q_dev, (size_t)B * idx->dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    CHECK(launch_prep(idx, s, B, (int)round_up(B, screen_tile(B)), idx->metric, ps.i8));
    std::vector<int> all(B);
    for (int i = 0; i < B; ++i) all[i] = i;
    if (m > 0) CHECK(run_scan(idx, s, ps, all, m, idx->subset_ids));
    hipLaunchKernelGGL(k_finalize, dim3(B), dim3(64), 0, s, idx->st, k, idx->row_offset, idx->view_row_map.p, out_dist_dev,
                       out_rows_dev, idx->status_or_dev, /*spec_metric=*/-1);
    HIPCHECK(idx, hipGetLastError());
    HIPCHECK(idx, hipMemcpyAsync(idx->status_host, idx->st.status, (size_t)kQBlockMax * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    // the scan re-runs every chunk that overflowed and clears the flag of each (complete_block, a pass that did not screen): one left over is a lost chunk
    for (int i = 0; i < B; ++i)
        if (idx->status_host[i] & kStOverflow)
            return fail(idx, MI355DR_E_INTERNAL, "subset scan: query " + std::to_string(i) + " lost a candidate chunk");
    return MI355DR_OK;
}

// ---- a block in flight -------------------------------------------------------------------------------------------------
// Round 3: a block no longer ends with a host synchronisation.  enqueue_block() puts the whole pass on the stream -- prepare,
// starter, chunks, finalize, a copy of the per-query status words into the block's own pinned buffer, an event -- and returns;
// complete_block() waits for the event and only then looks at the status: queries that overflowed a candidate list are
// re-screened (tighter bound, slower growth), queries the screen cannot rank are recomputed by the exact scan, each as a
// sub-block of its own whose results are scattered into the block's outputs.  Between the two calls the caller may enqueue
// the NEXT block (same stream): the GPU goes from one block's last kernel to the next one's first without waiting for the
// host's round trip (~50 us per block: 0.6 % of the 10 M-row pass, 4 % at the 8-way shard size).  The per-search state is
// single: blocks follow each other in stream order, and a fix-up (enqueued behind whatever is in flight) gathers its
// queries from the CALLER's buffer, which therefore stays valid until the wait.
int pending_alloc(mi355dr_index* idx, Pending& p) {
    HIPCHECK(idx, p.status_host.grow((kQBlockMax + 1) * sizeof(int)));
    HIPCHECK(idx, p.done.create(hipEventDisableTiming));
    return MI355DR_OK;
}

// level / force_scan: 0 / false for a caller's block; complete_block's fix-up passes say theirs
int enqueue_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int B, int k, double* out_dist_dev,
                  int64_t* out_rows_dev, Pending& p, int level = 0, bool force_scan = false) {
    CHECK(ensure_qstate(idx));
    CHECK(pending_alloc(idx, p));
    idx->last_pass_k = k;
    // a demoted int8 screen (AUTO) is on probation: first attempts at a demoted k count it down, then int8 gets another try
    if (level == 0 && idx->screen_dtype == MI355DR_SCREEN_AUTO && k >= idx->i8_demoted_k && --idx->i8_probation <= 0)
        idx->i8_demoted_k = INT_MAX;
    const int Bpad = (int)round_up(B, screen_tile(B));
    // (before the plan and the first launch: every kernel of the pass sees one screen type and one list stride)
    const Pass ps = decide_pass(idx, k, level, force_scan, "screen path unavailable (metric or too many irregular rows)");
    if (ps.refused) return fail(idx, MI355DR_E_UNSUPPORTED, ps.refused);
    // suspended speculation: passes that would have speculated count the probation down (this one takes the ladder)
    if (idx->spec_probation > 0 && ps.spec_eligible) idx->spec_probation--;
    if (q_dev != idx->qdev)
        HIPCHECK(idx, hipMemcpyAsync(idx->qdev, q_dev, (size_t)B * idx->dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    PassPlan plan;
    if (ps.screening) plan = make_plan(idx, ps, B);
    // (also re-arms the status word and the prune's hand-over counters, and starts the lists at the starter's count)
    CHECK(launch_prep(idx, s, B, Bpad, idx->metric, ps.i8, starter_count(plan)));
    if (idx->n > 0) {
        if (ps.screening) {
            CHECK(run_screen(idx, s, ps, B, plan));
        } else {
            std::vector<int> all(B);
            for (int i = 0; i < B; ++i) all[i] = i;
            CHECK(run_scan(idx, s, ps, all, idx->n));  // (blocks on the host only where a chunk larger than the buffer overflowed)
        }
    }
    // (a speculative pass is verified here: queries whose own k-th best does not justify the threshold they ran at are flagged)
    hipLaunchKernelGGL(k_finalize, dim3(B), dim3(64), 0, s, idx->st, k, idx->row_offset, idx->view_row_map.p, out_dist_dev,
                       out_rows_dev, idx->status_or_dev, ps.speculative && idx->n > 0 ? idx->metric : -1);
    HIPCHECK(idx, hipGetLastError());
    // (one copy: the per-query words and, behind them, their OR)
    HIPCHECK(idx, hipMemcpyAsync(p.status_host, idx->st.status, (size_t)(kQBlockMax + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipEventRecord(p.done, s));
    p.active = true;
    p.stream = s;
    p.q_dev = q_dev;
    p.B = B;
    p.pass = ps;
    p.out_dist = out_dist_dev;
    p.out_rows = out_rows_dev;
    return MI355DR_OK;
}

int search_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int B, int k, double* out_dist_dev,
                 int64_t* out_rows_dev, int level = 0, bool force_scan = false);

int complete_block(mi355dr_index* idx, Pending& p) {
    if (!p.active) return MI355DR_OK;
    p.active = false;
    HIPCHECK(idx, hipEventSynchronize(p.done));
    drain_events(idx);
    if (!p.pass.screening) {
        // the exact scan re-runs every chunk that overflowed (run_scan) and clears the flag of each: one left over is a lost chunk
        for (int i = 0; i < p.B; ++i)
            if (p.status_host[i] & kStOverflow)
                return fail(idx, MI355DR_E_INTERNAL, "exact scan: query " + std::to_string(i) + " lost a candidate chunk");
        return MI355DR_OK;
    }
    if (p.status_host[kQBlockMax] == 0) return MI355DR_OK;
    // some query overflowed its candidate buffer or has an irregular norm
    hipStream_t s = p.stream;
    const int B = p.B, k = p.pass.k, level = p.pass.level;
    std::vector<int> sub;  // [todo ... | retry ...]
    int n_todo = 0;
    {
        std::vector<int> retry;
        for (int i = 0; i < B; ++i) {
            const int st = p.status_host[i];
            if (st == 0) continue;
            if (p.pass.speculative && !(st & kStIrregular)) {  // (a speculative pass is level 0: these are re-run by the ladder)
                if (st & kStOverflow) idx->s_spec_overflow_queries++;
                else if (st & kStSpecMiss) idx->s_spec_miss_queries++;
            }
            // an overflow at the first attempt is re-screened with the tighter bound and slower growth; whatever
            // overflows again, and every query the screen cannot rank (irregular norm), is recomputed exactly
            if (level < kRetryLevels && !(st & kStIrregular)) retry.push_back(i);
            else sub.push_back(i);
        }
        n_todo = (int)sub.size();
        sub.insert(sub.end(), retry.begin(), retry.end());
    }
    const int n_sub = (int)sub.size(), n_retry = n_sub - n_todo;
    if (n_sub == 0) return MI355DR_OK;
    RetryBufs& rb = idx->retry[level];  // all four or no fix-up: a level whose set is incomplete asks again for what is missing
    HIPCHECK(idx, rb.q.grow((size_t)kQBlockMax * idx->dim * sizeof(float)));
    HIPCHECK(idx, rb.dist.grow((size_t)kQBlockMax * kKMax * sizeof(double)));
    HIPCHECK(idx, rb.rows.grow((size_t)kQBlockMax * kKMax * sizeof(int64_t)));
    HIPCHECK(idx, rb.map.grow((size_t)kQBlockMax * sizeof(int)));
    // both sub-blocks' queries are gathered from the caller's buffer BEFORE either runs (a nested search overwrites qdev)
    HIPCHECK(idx, hipMemcpyAsync(rb.map, sub.data(), n_sub * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gather_queries, dim3(n_sub), dim3(128), 0, s, p.q_dev, rb.map, idx->dim, rb.q);
    HIPCHECK(idx, hipGetLastError());
    HIPCHECK(idx, hipStreamSynchronize(s));  // `sub` (pageable) was read by the copy
    // guaranteed exact path (a pass of the next level, for its buffers; the scan itself never re-screens)
    if (n_todo > 0) CHECK(search_block(idx, s, rb.q, n_todo, k, rb.dist, rb.rows, level + 1, /*force_scan=*/true));
    if (n_retry > 0) {
        idx->s_retry_queries += n_retry;
        // AUTO gives the int8 screen up (from this k upwards) when more than 1 % of a block overflowed under its bound: the
        // re-screen is a bf16 pass of its own, and lists that overflow are lists that cost -- at d = 2048 (the int8 bound is
        // absolute, ~0.0175, the spread of the scores shrinks like 1 / sqrt(d)) 1.5 % of the queries overflowed and the pass
        // took 17.1 ms against 12.9 on bf16; at d = 768 nothing overflows.  (Round 2: 5 %.)
        // Not for ever -- a burst of queries into one dense neighbourhood must not cost a Gaussian-like corpus its int8 screen
        // (7.4 against 12.8 ms per block at the headline size): after 16 more blocks at such a k int8 gets another try, and the
        // wait doubles (up to 4096 blocks) whenever that try overflows again.
        // A speculative pass's misses and overflows speak of the MODEL, not of the int8 bound: they do not demote the screen.
        // More than 1 % of a block suspends speculation instead, the same way -- 16 first attempts, doubling up to 4096 with
        // every block that fails again, re-armed by option "speculate" -- so a corpus the model is wrong about costs one failed
        // block per probation period.  (Blocks already in flight finish as they were enqueued.)
        if (p.pass.speculative) {
            // (while suspended, a failing block is one that was in flight when the suspension began: the same verdict, not a
            // second one -- four blocks of one burst do not take the wait from 16 to 128)
            if (n_retry * 100 > B && idx->spec_probation <= 0) {
                idx->spec_backoff = idx->spec_backoff == 0 ? 16 : std::min(idx->spec_backoff * 2, 4096);
                idx->spec_probation = idx->spec_backoff;
            }
        } else if (p.pass.i8 && idx->screen_dtype == MI355DR_SCREEN_AUTO && n_retry * 100 > B) {
            idx->i8_demoted_k = std::min(idx->i8_demoted_k, k);
            idx->i8_backoff = idx->i8_backoff == 0 ? 16 : std::min(idx->i8_backoff * 2, 4096);
            idx->i8_probation = idx->i8_backoff;
        }
        CHECK(search_block(idx, s, rb.q + (size_t)n_todo * idx->dim, n_retry, k, rb.dist + (size_t)n_todo * k,
                           rb.rows + (size_t)n_todo * k, level + 1));
    }
    hipLaunchKernelGGL(k_scatter_results, dim3(n_sub), dim3(128), 0, s, rb.dist, rb.rows, rb.map, k, p.out_dist, p.out_rows);
    HIPCHECK(idx, hipGetLastError());
    HIPCHECK(idx, hipStreamSynchronize(s));
    return MI355DR_OK;
}

// blocks still in flight (mi355dr_search_device_async) are finished before anything that is not the next block on the same
// stream touches the per-search state or the corpus buffers
int complete_until(mi355dr_index* idx, int64_t seq) {  // finish the blocks below sequence number `seq`; the first error, if any
    int rc = MI355DR_OK;
    while (idx->seq_done < seq) {
        const int r = complete_block(idx, idx->pend[idx->seq_done % kPendingRing]);
        if (rc == MI355DR_OK) rc = r;
        idx->seq_done++;
    }
    return rc;
}
int drain_pending(mi355dr_index* idx) { return complete_until(idx, idx->seq_next); }

// one block of B <= kQBlockMax device-resident queries -> device outputs [B,k], complete on return
int search_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int B, int k, double* out_dist_dev,
                 int64_t* out_rows_dev, int level, bool force_scan) {
    Pending& p = idx->sub_pend[std::min(level, kRetryLevels + 1)];
    CHECK(enqueue_block(idx, s, q_dev, B, k, out_dist_dev, out_rows_dev, p, level, force_scan));
    return complete_block(idx, p);
}

// k_merge_topk sorts next_pow2(world * k) entries: LDS and threads by need (80 entries at 8 ranks x k = 10 -- a 256-thread
// workgroup with 48 KiB of LDS per query kept the merge from slipping in beside other work)
inline size_t merge_lds(int world, int k) {
    size_t np = 1;
    while (np < (size_t)world * k) np <<= 1;
    return np * 12;
}
inline int merge_threads(int world, int k) { return (int64_t)world * k <= 128 ? 64 : 256; }

// rank r's [B, k] distances / rows start r * stride entries behind dist_all / rows_all; asynchronous on the stream
int launch_merge(mi355dr_index* idx, const double* dist_all, const int64_t* rows_all, int64_t stride, int world, int B, int k,
                 double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    if (world <= 0 || B < 0 || k <= 0) return fail(idx, MI355DR_E_INVALID, "bad merge shape");
    if ((int64_t)world * k > kSortMax) return fail(idx, MI355DR_E_UNSUPPORTED, "world*k exceeds 4096");
    if (B == 0) return MI355DR_OK;
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(ensure_qstate(idx));
    hipStream_t s = stream ? (hipStream_t)stream : idx->stream;
    hipLaunchKernelGGL(k_merge_topk, dim3(B), dim3(merge_threads(world, k)), merge_lds(world, k), s, dist_all, rows_all, stride,
                       world, B, k, out_dist_dev, out_rows_dev);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// the start of the debug entry points and of a host pair list (rescore_host_pairs): blocks in flight finished, the B queries uploaded and prepared (`metric`: k_prep_queries)
int upload_and_prep(mi355dr_index* idx, const float* queries, int B, int metric) {
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_pending(idx));
    CHECK(ensure_qstate(idx));
    HIPCHECK(idx, hipMemcpyAsync(idx->qdev, queries, (size_t)B * idx->dim * sizeof(float), hipMemcpyHostToDevice, idx->stream));
    return launch_prep(idx, idx->stream, B, (int)round_up(B, screen_tile(B)), metric, idle_i8(idx));
}

int check_search_args(mi355dr_index* idx, const void* q, int B, int k, const void* od, const void* orow) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    if (B < 0 || k <= 0) return fail(idx, MI355DR_E_INVALID, "B must be >= 0 and k > 0");
    if (k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "k exceeds 1024");
    if (B > 0 && (!q || !od || !orow)) return fail(idx, MI355DR_E_INVALID, "null buffer");
    return MI355DR_OK;
}

int check_radii(mi355dr_index* idx, const std::string& what, const double* radius, int B) {
    for (int b = 0; b < B; ++b)
        if (radius[b] != radius[b]) return fail(idx, MI355DR_E_INVALID, what + ": radius " + std::to_string(b) + " is NaN");
    return MI355DR_OK;
}

// ---- the call frame of the search entry points ---------------------------------------------------------------------------
// begin_call(), in this order: null handle; a view refuses (kCallNoView; is_view is set once, before the handle is handed
// out); the call's own argument checks (`args_ok`: nothing has been touched when they fail); the handle's mutex, held until
// `c` leaves; the device; blocks in flight finished (kCallDrain: they complete, and their errors surface, on an empty call too);
// the caller's stream or the handle's; the per-search state.  The empty-call return is the caller's, behind this.
enum : unsigned { kCallNoView = 1, kCallDrain = 2 };
struct Call {
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
};
template <class ArgCheck>
int begin_call(mi355dr_index* idx, const char* what, void* stream, unsigned flags, Call& c, ArgCheck&& args_ok) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    if ((flags & kCallNoView) && idx->is_view) return view_refuses(idx, what, /*ask_parent=*/true);
    CHECK(args_ok());
    c.lock = std::unique_lock<std::mutex>(idx->mu);
    HIPCHECK(idx, hipSetDevice(idx->device));
    if (flags & kCallDrain) CHECK(drain_pending(idx));
    c.s = stream ? (hipStream_t)stream : idx->stream;
    return ensure_qstate(idx);
}

// ---- one call's queries and results, block by block ------------------------------------------------------------------------
// host == true: the caller's buffers are host memory -- a block's queries are staged through idx->qdev, its results through
// the handle's one result staging (index.h: out_*_dev); else they are device memory used in place.  `width`: entries per
// result line; `count` (int64, the grouped search's int32): null when the call has none.
template <class Count>
struct BlockOut {
    double* dist;
    int64_t* rows;
    Count* count;
};
template <class Count = int64_t>
struct CallIO {
    bool host;
    hipStream_t s;
    const float* q;       // the caller's queries [B, dim] (null: the call brings none)
    BlockOut<Count> out;  // the caller's results [B, width] / [B]
    int width;
};

// the device pointer of queries [b0, b0 + nb) (host form: uploaded behind whatever still reads qdev on the stream)
template <class Count>
int block_queries(mi355dr_index* idx, const CallIO<Count>& io, int b0, int nb, const float** q_dev) {
    *q_dev = io.q + (int64_t)b0 * idx->dim;
    if (!io.host) return MI355DR_OK;
    HIPCHECK(idx, hipMemcpyAsync(idx->qdev, *q_dev, (size_t)nb * idx->dim * sizeof(float), hipMemcpyHostToDevice, io.s));
    *q_dev = idx->qdev;
    return MI355DR_OK;
}

// where the kernels write the results of the block that starts at b0
BlockOut<int64_t> block_outputs(mi355dr_index* idx, const CallIO<>& io, int b0) {
    if (io.host) return {idx->out_dist_dev, idx->out_rows_dev, io.out.count ? idx->out_count_dev.p : nullptr};
    return {io.out.dist + (int64_t)b0 * io.width, io.out.rows + (int64_t)b0 * io.width, io.out.count ? io.out.count + b0 : nullptr};
}

// host form: the block's nb lines (and counts) from where they were staged (`o`) to the caller's, asynchronous on the
// stream; device form: they are in place
template <class Count>
int block_return(mi355dr_index* idx, const CallIO<Count>& io, int b0, int nb, const BlockOut<Count>& o) {
    if (!io.host) return MI355DR_OK;
    const size_t n = (size_t)nb * io.width;
    HIPCHECK(idx, hipMemcpyAsync(io.out.dist + (int64_t)b0 * io.width, o.dist, n * sizeof(double), hipMemcpyDeviceToHost, io.s));
    HIPCHECK(idx, hipMemcpyAsync(io.out.rows + (int64_t)b0 * io.width, o.rows, n * sizeof(int64_t), hipMemcpyDeviceToHost, io.s));
    if (o.count) HIPCHECK(idx, hipMemcpyAsync(io.out.count + b0, o.count, (size_t)nb * sizeof(Count), hipMemcpyDeviceToHost, io.s));
    return MI355DR_OK;
}

// ---- exact distances of listed (query, row) pairs ---------------------------------------------------------------------------
// the pairs' queries are the prepared block in qdev; k_rescore_pairs does not range-check: rows are local and inside the index
int launch_rescore(mi355dr_index* idx, hipStream_t s, const int32_t* pair_q_dev, const int64_t* pair_row_dev, int64_t n_pairs,
                   float* dot_dev, double* dist_dev) {
    hipLaunchKernelGGL(k_rescore_pairs, dim3((unsigned)((n_pairs + kWave - 1) / kWave)), dim3(kWave), 0, s, idx->rows, idx->nrm2,
                       idx->qdev, idx->st.qn, pair_q_dev, pair_row_dev, n_pairs, idx->dim, idx->metric, dot_dev, dist_dev);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// the same for pairs listed on the host, against a block of B host queries: blocks in flight finished, the queries uploaded
// and prepared, the lists uploaded, the distances (out_dot != null: and the dots) back in the caller's arrays on return.
// `bufs` is the caller's local: it grows with the largest list of the call and leaves with it.
struct PairBufs {
    DevBuf<int32_t> q;
    DevBuf<int64_t> row;
    DevBuf<float> dot;
    DevBuf<double> dist;
};
int rescore_host_pairs(mi355dr_index* idx, PairBufs& bufs, const float* queries, int B, const int32_t* pair_q,
                       const int64_t* pair_row, int64_t n_pairs, float* out_dot, double* out_dist) {
    hipStream_t s = idx->stream;
    CHECK(upload_and_prep(idx, queries, B, idx->metric));
    HIPCHECK(idx, grow_each(n_pairs, bufs.q, bufs.row, bufs.dot, bufs.dist));
    HIPCHECK(idx, hipMemcpyAsync(bufs.q.p, pair_q, n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipMemcpyAsync(bufs.row.p, pair_row, n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, s));
    CHECK(launch_rescore(idx, s, bufs.q.p, bufs.row.p, n_pairs, bufs.dot.p, bufs.dist.p));
    if (out_dot) HIPCHECK(idx, hipMemcpyAsync(out_dot, bufs.dot.p, n_pairs * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(out_dist, bufs.dist.p, n_pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    return MI355DR_OK;
}

}  // namespace

namespace mi355 {
int drain_searches(mi355dr_index* idx) { return drain_pending(idx); }
int merge_topk_reserve(mi355dr_index* idx) { return ensure_qstate(idx); }
int merge_topk_packed(mi355dr_index* idx, const int64_t* packed_all_dev, int world, int B, int k, double* out_dist_dev,
                      int64_t* out_rows_dev, hipStream_t stream) {
    const int64_t plane = (int64_t)B * k;
    return launch_merge(idx, (const double*)packed_all_dev, packed_all_dev + plane, 2 * plane, world, B, k, out_dist_dev, out_rows_dev,
                        stream);
}
}  // namespace mi355

extern "C" {

int mi355dr_version(void) { return 102; }

const char* mi355dr_last_error(const mi355dr_index* idx) {
    if (idx) return idx->err.c_str();
    std::lock_guard<std::mutex> g(g_err_mu);
    return g_err.c_str();
}

int mi355dr_create(mi355dr_index** out, int device_id, int dim, int metric) {
    if (!out) return fail(nullptr, MI355DR_E_INVALID, "out is null");
    *out = nullptr;
    if (dim <= 0 || dim > 16384) return fail(nullptr, MI355DR_E_INVALID, "dim must be in [1,16384]");
    if (metric != MI355DR_METRIC_COSINE && metric != MI355DR_METRIC_IP)
        return fail(nullptr, MI355DR_E_INVALID, "metric must be 0 (cosine) or 1 (inner product)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, MI355DR_E_HIP, "no HIP device available (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, MI355DR_E_INVALID, "device_id out of range");
    mi355dr_index* idx = new mi355dr_index();
    idx->device = device_id;
    idx->dim = dim;
    idx->dpad = (int)round_up(dim, kStepK);
    idx->dpad8 = (int)round_up(dim, kRowB);
    idx->metric = metric;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking);
    auto zeroed = [&](auto& word) {  // one 4-byte counter or running maximum, starting at 0
        if (e == hipSuccess) e = word.grow(4);
        if (e == hipSuccess) e = hipMemset(word, 0, 4);
    };
    if (e == hipSuccess) e = idx->irr_rows.grow(kIrrCap * sizeof(int32_t));
    zeroed(idx->irr_count);
    zeroed(idx->n2max_dev);
    zeroed(idx->bf16_res2_dev);
    if (e == hipSuccess) e = idx->irr8_rows.grow(kIrrCap * sizeof(int32_t));
    zeroed(idx->irr8_count);
    zeroed(idx->dead_count);
    if (e == hipSuccess) e = idx->t0.create();
    if (e == hipSuccess) e = idx->t1.create();
    if (e != hipSuccess) {
        std::string m = std::string("device setup failed: ") + hipGetErrorString(e);
        delete idx;  // (its members and its destructor release whatever the steps before the failure created)
        return fail(nullptr, MI355DR_E_HIP, m);
    }
    *out = idx;
    return MI355DR_OK;
}

void mi355dr_destroy(mi355dr_index* idx) {
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    (void)drain_pending(idx);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    multivec_destroy(idx);
    sparse_destroy(idx);
    comm_destroy(idx);
    delete idx;  // every buffer and event goes with its owner, the stream with the handle's destructor (index.h)
}

int mi355dr_reserve(mi355dr_index* idx, int64_t n_rows) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "reserve");
    HIPCHECK(idx, hipSetDevice(idx->device));
    if (n_rows < 0) return fail(idx, MI355DR_E_INVALID, "negative row count");
    if (n_rows >= (int64_t)1 << 31) return fail(idx, MI355DR_E_UNSUPPORTED, "more than 2^31-1 rows per index");
    CHECK(drain_pending(idx));
    return ensure_capacity(idx, n_rows);
}

// ---- the derived data of stored rows: built and published the same way by add, update and remove ------------------------
namespace {
// the per-row build kernels run one workgroup per row: a grid is kept below 2^22 rows (gridDim.x * blockDim.x < 2^32)
constexpr int64_t kBuildSlice = (int64_t)1 << 22;

// |c|^2 (with_nrm2) and the bf16 image of n rows: [first, first + n), or ids[0 .. n) (device) when ids != nullptr
int build_rows(mi355dr_index* idx, hipStream_t s, int64_t first, int64_t n, const int64_t* ids, bool with_nrm2) {
    for (int64_t r0 = 0; r0 < n; r0 += kBuildSlice) {
        const int64_t m = std::min(kBuildSlice, n - r0), row0 = ids ? 0 : first + r0;
        const int64_t* slice = ids ? ids + r0 : nullptr;
        if (with_nrm2) {
            hipLaunchKernelGGL(k_row_nrm2, dim3((unsigned)((m + kWave - 1) / kWave)), dim3(kWave), 0, s, idx->rows, row0, m,
                               idx->dim, idx->nrm2, idx->n2max_dev, slice);
            HIPCHECK(idx, hipGetLastError());
        }
        hipLaunchKernelGGL(k_build_shadow, dim3((unsigned)m), dim3(256), 0, s, idx->rows, idx->nrm2, row0, m, idx->dim,
                           idx->dpad, idx->shadow, idx->irr_rows, idx->irr_count, idx->bf16_res2_dev,
                           idx->metric == MI355DR_METRIC_IP ? 1 : 0, slice);
        HIPCHECK(idx, hipGetLastError());
    }
    return MI355DR_OK;
}

// the int8 image of n whole groups of 32 rows: [g_first, g_first + n), or groups[0 .. n) (device) when groups != nullptr
// (n_total, first_new: k_build_shadow8 -- loose rows from first_new on are appended to their side list)
int build_groups(mi355dr_index* idx, hipStream_t s, int64_t g_first, int64_t n, const int64_t* groups, int64_t n_total,
                 int64_t first_new) {
    for (int64_t g0 = 0; g0 < n; g0 += kBuildSlice) {
        const int64_t m = std::min(kBuildSlice, n - g0);
        hipLaunchKernelGGL(k_build_shadow8, dim3((unsigned)m), dim3(256), 0, s, idx->rows, idx->nrm2, groups ? 0 : g_first + g0,
                           n_total, first_new, idx->dim, idx->dpad8, idx->shadow8, idx->flag8, idx->grp8, idx->irr8_rows,
                           idx->irr8_count, idx->metric == MI355DR_METRIC_IP ? 1 : 0, groups ? groups + g0 : nullptr);
        HIPCHECK(idx, hipGetLastError());
    }
    return MI355DR_OK;
}

// what the build kernels counted and measured becomes the host's view of the corpus; the call's one synchronisation
int commit_corpus(mi355dr_index* idx, hipStream_t s, bool mutated) {
    int irr = 0, irr8 = 0, dead = 0;
    float res2 = 0.0f, n2max = 0.0f;
    HIPCHECK(idx, hipMemcpyAsync(&irr, idx->irr_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(&irr8, idx->irr8_count, sizeof(int), hipMemcpyDeviceToHost, s));
    if (mutated) HIPCHECK(idx, hipMemcpyAsync(&dead, idx->dead_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(&res2, idx->bf16_res2_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(&n2max, idx->n2max_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    // the two running maxima only ever grow (the row that held one may be gone: a looser bound is still a bound)
    idx->cmax = std::sqrt(n2max) * 1.000001f;
    // (a-priori cap: 2^-8 |c_hat|; inner product: the shadow holds the rows themselves, residuals in their units)
    idx->bf16_ec = std::min(std::sqrt(res2) * 1.001f, 0.00390625f * 1.0001f * (idx->metric == MI355DR_METRIC_IP ? idx->cmax : 1.0f));
    idx->irr_n = irr;
    idx->irr8_n = irr8;
    if (mutated) idx->dead_n = dead;
    return MI355DR_OK;
}
}  // namespace

static int add_rows_impl(mi355dr_index* idx, const float* rows, int64_t n, hipMemcpyKind kind) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "add_rows");
    if (n < 0) return fail(idx, MI355DR_E_INVALID, "negative row count");
    if (n == 0) return MI355DR_OK;
    if (!rows) return fail(idx, MI355DR_E_INVALID, "rows is null");
    if (idx->n + n >= (int64_t)1 << 31) return fail(idx, MI355DR_E_UNSUPPORTED, "more than 2^31-1 rows per index");
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_pending(idx));
    CHECK(ensure_capacity(idx, idx->n + n));
    hipStream_t s = idx->stream;
    HIPCHECK(idx, hipMemcpyAsync(idx->rows + idx->n * idx->dim, rows, (size_t)n * idx->dim * sizeof(float), kind, s));
    CHECK(build_rows(idx, s, idx->n, n, nullptr, /*with_nrm2=*/true));
    // int8 shadow: whole groups of 32 rows, from the (possibly partly filled) group the first new row falls into
    const int64_t g_lo = idx->n / kI8GroupRows, g_hi = (idx->n + n + kI8GroupRows - 1) / kI8GroupRows;
    CHECK(build_groups(idx, s, g_lo, g_hi - g_lo, nullptr, idx->n + n, idx->n));
    CHECK(commit_corpus(idx, s, /*mutated=*/false));
    idx->n += n;
    return MI355DR_OK;
}

int mi355dr_add_rows(mi355dr_index* idx, const float* rows, int64_t n) {
    return add_rows_impl(idx, rows, n, hipMemcpyHostToDevice);
}
int mi355dr_add_rows_device(mi355dr_index* idx, const float* rows_dev, int64_t n) {
    return add_rows_impl(idx, rows_dev, n, hipMemcpyDeviceToDevice);
}

// ---- update / remove in place (DESIGN.md "Mutable index") ---------------------------------------------------------------
namespace {
constexpr int64_t kMutSlice = (int64_t)1 << 16;  // rows per staging upload and per-row launch

// rows == nullptr: remove.  kind: where `rows` lives.  row_ids: host.
int mutate_rows_impl(mi355dr_index* idx, const int64_t* row_ids, const float* rows, int64_t n, hipMemcpyKind kind, bool remove) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, remove ? "remove_rows" : "update_rows");
    if (n < 0) return fail(idx, MI355DR_E_INVALID, "negative row count");
    if (n == 0) {  // (nothing to change, but the ordering promise holds: what is in flight is complete on return)
        HIPCHECK(idx, hipSetDevice(idx->device));
        return drain_pending(idx);
    }
    if (!row_ids || (!remove && !rows)) return fail(idx, MI355DR_E_INVALID, "null argument");
    // every id inside the index and listed once -- checked before anything is touched
    std::vector<int64_t> sorted(row_ids, row_ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= idx->n) return fail(idx, MI355DR_E_INVALID, "row id out of range");
    for (int64_t i = 1; i < n; ++i)
        if (sorted[i] == sorted[i - 1]) return fail(idx, MI355DR_E_INVALID, "duplicated row id " + std::to_string(sorted[i]));
    std::vector<int64_t> groups;  // the int8 groups the call touches, each once
    for (int64_t r : sorted)
        if (groups.empty() || groups.back() != r / kI8GroupRows) groups.push_back(r / kI8GroupRows);
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_pending(idx));  // (a search in flight sees the index as it was)
    hipStream_t s = idx->stream;
    DevBuf<void> ids_dev, groups_dev, stage;  // scratch of one call, released on every way out
    HIPCHECK(idx, ids_dev.grow((size_t)n * sizeof(int64_t)));
    HIPCHECK(idx, groups_dev.grow(groups.size() * sizeof(int64_t)));
    HIPCHECK(idx, hipMemcpyAsync(ids_dev.p, row_ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipMemcpyAsync(groups_dev.p, groups.data(), groups.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (!remove && kind == hipMemcpyHostToDevice)
        HIPCHECK(idx, stage.grow((size_t)std::min(n, kMutSlice) * idx->dim * sizeof(float)));
    for (int64_t r0 = 0; r0 < n; r0 += kMutSlice) {
        const int64_t m = std::min(kMutSlice, n - r0);
        const int64_t* ids = (const int64_t*)ids_dev.p + r0;
        if (remove) {
            hipLaunchKernelGGL(k_mark_dead, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, ids, m, idx->nrm2);
            HIPCHECK(idx, hipGetLastError());
        } else {
            const float* src = rows + r0 * idx->dim;
            if (stage.p) {
                HIPCHECK(idx, hipMemcpyAsync(stage.p, src, (size_t)m * idx->dim * sizeof(float), hipMemcpyHostToDevice, s));
                src = (const float*)stage.p;
            }
            const int vec4 = idx->dim % 4 == 0 && (uintptr_t)src % 16 == 0;
            hipLaunchKernelGGL(k_update_rows, dim3((unsigned)m), dim3(256), 0, s, src, ids, m, idx->dim, vec4, idx->rows);
            HIPCHECK(idx, hipGetLastError());
        }
        CHECK(build_rows(idx, s, 0, m, ids, /*with_nrm2=*/!remove));
    }
    CHECK(build_groups(idx, s, 0, (int64_t)groups.size(), (const int64_t*)groups_dev.p, idx->n, idx->n));
    // both side lists and the dead count anew, from the flags (a row may have entered or left either class)
    HIPCHECK(idx, hipMemsetAsync(idx->irr_count, 0, sizeof(int), s));
    HIPCHECK(idx, hipMemsetAsync(idx->irr8_count, 0, sizeof(int), s));
    HIPCHECK(idx, hipMemsetAsync(idx->dead_count, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_rebuild_side_lists, dim3((unsigned)((idx->n + 255) / 256)), dim3(256), 0, s, idx->nrm2, idx->flag8,
                       (int64_t)0, idx->n, idx->irr_rows, idx->irr_count, idx->irr8_rows, idx->irr8_count, idx->dead_count);
    HIPCHECK(idx, hipGetLastError());
    return commit_corpus(idx, s, /*mutated=*/true);
}
}  // namespace

int mi355dr_update_rows(mi355dr_index* idx, const int64_t* row_ids, const float* rows, int64_t n) {
    return mutate_rows_impl(idx, row_ids, rows, n, hipMemcpyHostToDevice, false);
}
int mi355dr_update_rows_device(mi355dr_index* idx, const int64_t* row_ids, const float* rows_dev, int64_t n) {
    return mutate_rows_impl(idx, row_ids, rows_dev, n, hipMemcpyDeviceToDevice, false);
}
int mi355dr_remove_rows(mi355dr_index* idx, const int64_t* row_ids, int64_t n) {
    return mutate_rows_impl(idx, row_ids, nullptr, n, hipMemcpyHostToDevice, true);
}

// ---- compaction (DESIGN.md "Compaction") --------------------------------------------------------------------------------
int mi355dr_compact(mi355dr_index* idx, int64_t* new_of_old) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "compact");
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_pending(idx));  // (a search in flight sees the index as it was, under the old ids)
    const int64_t n_old = idx->n;
    if (idx->dead_n == 0) {  // nothing to drop: nothing is read, moved or rebuilt
        if (new_of_old)
            for (int64_t r = 0; r < n_old; ++r) new_of_old[r] = r;
        return MI355DR_OK;
    }
    hipStream_t s = idx->stream;
    // the dead rows from nrm2; src_of_dst for the destinations from the first dead slot on (rows in front of it stay)
    std::vector<float> n2;
    std::vector<int32_t> src_of_dst;
    int64_t first_dead = n_old;
    try {
        n2.resize((size_t)n_old);
        HIPCHECK(idx, hipMemcpyAsync(n2.data(), idx->nrm2, (size_t)n_old * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHECK(idx, hipStreamSynchronize(s));
        for (int64_t r = 0; r < n_old; ++r)
            if (row_is_dead(n2[(size_t)r])) {
                first_dead = r;
                break;
            }
        src_of_dst.reserve((size_t)(n_old - first_dead));
        for (int64_t r = first_dead; r < n_old; ++r)
            if (!row_is_dead(n2[(size_t)r])) src_of_dst.push_back((int32_t)r);
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "compact: out of host memory for the row maps");
    }
    const int64_t n_moved = (int64_t)src_of_dst.size(), n_new = first_dead + n_moved;
    const int64_t slice = std::min(idx->compact_slice_rows, n_moved);
    const size_t row_b = (size_t)idx->dim * sizeof(float);
    // every allocation of the call, before the first byte of the index is written
    DevBuf<int32_t> map_dev;
    DevBuf<float> stage;  // [slice, dim] rows, then [slice] nrm2
    // (src_of_dst is pageable: HIP stages such a copy before the call returns, as for the id lists of mutate_rows_impl, and
    // commit_corpus synchronises the stream before the vector goes)
    if (n_moved > 0) {
        HIPCHECK(idx, map_dev.grow((size_t)n_moved * sizeof(int32_t)));
        HIPCHECK(idx, stage.grow((size_t)slice * (row_b + sizeof(float))));
        HIPCHECK(idx, hipMemcpyAsync(map_dev.p, src_of_dst.data(), (size_t)n_moved * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    float* stage_n2 = stage.p + slice * idx->dim;
    const int vec4 = idx->dim % 4 == 0 && (uintptr_t)idx->rows.p % 16 == 0 && (uintptr_t)stage.p % 16 == 0;
    for (int64_t j0 = 0; j0 < n_moved; j0 += slice) {  // ascending slices of destination rows first_dead + [j0, j0 + m)
        const int64_t m = std::min(slice, n_moved - j0), dst0 = first_dead + j0;
        hipLaunchKernelGGL(k_compact_gather, dim3((unsigned)((m + kCompactWaves - 1) / kCompactWaves)), dim3(64 * kCompactWaves),
                           0, s, idx->rows, idx->nrm2, map_dev.p + j0, m, idx->dim, vec4, stage.p, stage_n2);
        HIPCHECK(idx, hipGetLastError());
        HIPCHECK(idx, hipMemcpyAsync(idx->rows + dst0 * idx->dim, stage.p, (size_t)m * row_b, hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(idx->nrm2 + dst0, stage_n2, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    // the slots behind the new end, up to the end of the last 256-row tile the old index reached, become capacity that was
    // never used (ensure_capacity: all-zero images, flags and group records) -- screens read whole tiles and whole groups
    const int64_t tail_end = std::min(round_up(n_old, kT2), idx->cap_rows), tail = tail_end - n_new;
    const int64_t g_tail = (n_new + kI8GroupRows - 1) / kI8GroupRows, g_end = tail_end / kI8GroupRows;
    if (tail > 0) {
        HIPCHECK(idx, hipMemsetAsync(idx->nrm2 + n_new, 0, (size_t)tail * sizeof(float), s));
        HIPCHECK(idx, hipMemsetAsync(idx->shadow + n_new * idx->dpad, 0, (size_t)tail * idx->dpad * sizeof(uint16_t), s));
        HIPCHECK(idx, hipMemsetAsync(idx->shadow8 + n_new * idx->dpad8, 0, (size_t)tail * idx->dpad8, s));
        HIPCHECK(idx, hipMemsetAsync(idx->flag8 + n_new, 0, (size_t)tail, s));
    }
    if (g_end > g_tail) HIPCHECK(idx, hipMemsetAsync(idx->grp8 + g_tail, 0, (size_t)(g_end - g_tail) * sizeof(I8Group), s));
    // derived data of the moved rows, by the builders add_rows uses (nrm2 came with the rows: the bits of their add)
    CHECK(build_rows(idx, s, first_dead, n_moved, nullptr, /*with_nrm2=*/false));
    const int64_t g_lo = first_dead / kI8GroupRows;  // group membership shifts from here on: whole groups, as an append rebuilds them
    CHECK(build_groups(idx, s, g_lo, g_tail - g_lo, nullptr, n_new, n_new));
    HIPCHECK(idx, hipMemsetAsync(idx->irr_count, 0, sizeof(int), s));
    HIPCHECK(idx, hipMemsetAsync(idx->irr8_count, 0, sizeof(int), s));
    HIPCHECK(idx, hipMemsetAsync(idx->dead_count, 0, sizeof(int), s));
    if (n_new > 0) {
        hipLaunchKernelGGL(k_rebuild_side_lists, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, s, idx->nrm2, idx->flag8,
                           (int64_t)0, n_new, idx->irr_rows, idx->irr_count, idx->irr8_rows, idx->irr8_count, idx->dead_count);
        HIPCHECK(idx, hipGetLastError());
    }
    CHECK(commit_corpus(idx, s, /*mutated=*/true));
    idx->n = n_new;
    // AUTO's demotion of the int8 screen was a verdict on the old layout (a dead head overflows every int8 list): re-armed, as
    // setting "screen_dtype" does
    idx->i8_demoted_k = INT_MAX;
    idx->i8_backoff = idx->i8_probation = 0;
    idx->spec_backoff = idx->spec_probation = 0;  // (so was a suspended speculation: the sample is of other rows now)
    idx->s_compactions += n_moved > 0;  // (a call that only dropped a dead tail moved nothing)
    idx->s_compact_moved_rows += n_moved;
    if (new_of_old) {
        int64_t next = 0;
        for (int64_t r = 0; r < n_old; ++r) new_of_old[r] = row_is_dead(n2[(size_t)r]) ? -1 : next++;
    }
    return MI355DR_OK;
}

// ---- views (DESIGN.md section 4.8c "Views") --------------------------------------------------------------------------------
namespace {
// a call on the view that failed: the caller asks the PARENT for the text
#define VIEWCHECK(parent, view, expr)                                                         \
    do {                                                                                      \
        int rc__ = (expr);                                                                    \
        if (rc__ != MI355DR_OK) return fail(parent, rc__, "view_create: " + (view)->err);     \
    } while (0)

// the caller's global ids -> `out`: local, ascending, unique (subset_ids.h: the rule of mi355dr_search_subset)
int view_local_ids(mi355dr_index* parent, const int64_t* ids, int64_t m, int64_t n, std::vector<int32_t>& out) {
    try {
        subset_prepare_ids(ids, m, parent->row_offset, n, out);
    } catch (const std::bad_alloc&) {
        return fail(parent, MI355DR_E_NOMEM, "view_create: out of host memory for the id list");
    }
    return MI355DR_OK;
}

// `local` + the parent's row_offset -> a device map the view owns
int view_upload_map(mi355dr_index* parent, const std::vector<int32_t>& local, DevBuf<int64_t>& map) {
    if (local.empty()) return MI355DR_OK;
    std::vector<int64_t> global;
    try {
        global.resize(local.size());
    } catch (const std::bad_alloc&) {
        return fail(parent, MI355DR_E_NOMEM, "view_create: out of host memory for the id map");
    }
    for (size_t j = 0; j < local.size(); ++j) global[j] = (int64_t)local[j] + parent->row_offset;
    HIPCHECK(parent, map.grow(global.size() * sizeof(int64_t)));
    HIPCHECK(parent, hipMemcpy(map.p, global.data(), global.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return MI355DR_OK;
}

// Everything between the view's creation and its publication; the caller destroys the view when this fails.  The parent's
// mutex is held and nothing of the parent is written.  Gathers run on the PARENT's stream and are waited for on the host
// before the view's add path (its own stream, complete on return) reads the staging buffer -- one synchronisation per slice.
int view_build(mi355dr_index* parent, mi355dr_index* view, const int64_t* row_ids, int64_t m_rows, const int64_t* doc_ids,
               int64_t m_docs) {
    hipStream_t s = parent->stream;
    const int d = parent->dim;
    const size_t row_b = (size_t)d * sizeof(float);
    const int64_t slice = parent->view_slice_rows;  // rows -- and tokens: the token slices have the same byte count
    // ---- the lists: local, ascending, unique; removed rows and documents without vectors leave
    std::vector<int32_t> rows, docs;
    CHECK(view_local_ids(parent, row_ids, m_rows, parent->n, rows));
    DevBuf<int32_t> ids_dev;
    if (!rows.empty()) {
        HIPCHECK(parent, ids_dev.grow(rows.size() * sizeof(int32_t)));
        HIPCHECK(parent, hipMemcpyAsync(ids_dev.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHECK(parent, hipStreamSynchronize(s));
    }
    if (!rows.empty() && parent->dead_n > 0) {  // the m norms are read back (4 m bytes) and the dead rows dropped on the host
        const int64_t m = (int64_t)rows.size();
        DevBuf<float> n2_dev;
        std::vector<float> n2;
        try {
            n2.resize((size_t)m);
        } catch (const std::bad_alloc&) {
            return fail(parent, MI355DR_E_NOMEM, "view_create: out of host memory for the listed rows' norms");
        }
        HIPCHECK(parent, n2_dev.grow((size_t)m * sizeof(float)));
        hipLaunchKernelGGL(k_view_gather_nrm2, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, parent->nrm2.p, ids_dev.p, m, n2_dev.p);
        HIPCHECK(parent, hipGetLastError());
        HIPCHECK(parent, hipMemcpyAsync(n2.data(), n2_dev.p, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHECK(parent, hipStreamSynchronize(s));
        int64_t keep = 0;
        for (int64_t j = 0; j < m; ++j)
            if (!row_is_dead(n2[(size_t)j])) rows[(size_t)keep++] = rows[(size_t)j];
        if (keep < m) {
            rows.resize((size_t)keep);
            if (keep > 0) {
                HIPCHECK(parent, hipMemcpyAsync(ids_dev.p, rows.data(), (size_t)keep * sizeof(int32_t), hipMemcpyHostToDevice, s));
                HIPCHECK(parent, hipStreamSynchronize(s));
            }
        }
    }
    MultiVecView pv{};
    if (m_docs > 0 && multivec_view(parent, &pv)) {
        CHECK(view_local_ids(parent, doc_ids, m_docs, pv.n_docs, docs));
        docs.erase(std::remove_if(docs.begin(), docs.end(), [&](int32_t i) { return pv.tok_cnt_host[i] <= 0; }), docs.end());
    }
    const int64_t n_rows = (int64_t)rows.size(), n_docs = (int64_t)docs.size();
    // ---- the one staging buffer: a slice of rows, or a slice of tokens (a document longer than a slice goes alone)
    int64_t tok_total = 0, tok_longest = 0, blk_total = 0;
    for (int32_t i : docs) {
        const int64_t T = pv.tok_cnt_host[i];
        tok_total += T;
        tok_longest = std::max(tok_longest, T);
        blk_total += (T + kMsBlkRows - 1) / kMsBlkRows;
    }
    const int64_t stage_rows = std::max(std::min(slice, n_rows), std::max(std::min(slice, tok_total), tok_longest));
    DevBuf<float> stage;
    if (stage_rows > 0) HIPCHECK(parent, stage.grow((size_t)stage_rows * row_b));
    // ---- single-vector rows
    if (n_rows > 0) {
        VIEWCHECK(parent, view, mi355dr_reserve(view, n_rows));
        const int vec4 = d % 4 == 0 && (uintptr_t)parent->rows.p % 16 == 0 && (uintptr_t)stage.p % 16 == 0;
        for (int64_t j0 = 0; j0 < n_rows; j0 += slice) {
            const int64_t m = std::min(slice, n_rows - j0);
            hipLaunchKernelGGL(k_view_gather_rows, dim3((unsigned)((m + kViewWaves - 1) / kViewWaves)), dim3(64 * kViewWaves), 0, s,
                               parent->rows.p, ids_dev.p + j0, m, d, vec4, stage.p);
            HIPCHECK(parent, hipGetLastError());
            HIPCHECK(parent, hipStreamSynchronize(s));
            VIEWCHECK(parent, view, mi355dr_add_rows_device(view, stage.p, m));
        }
        CHECK(view_upload_map(parent, rows, view->view_row_map));
    }
    // ---- documents
    if (n_docs > 0) {
        VIEWCHECK(parent, view, multivec_reserve(view, blk_total, n_docs));
        std::vector<ViewTokBlock> blocks;
        std::vector<int64_t> offsets;
        DevBuf<ViewTokBlock> blocks_dev;
        for (int64_t i0 = 0, i1; i0 < n_docs; i0 = i1) {
            blocks.clear();
            offsets.assign(1, 0);
            try {
                for (i1 = i0; i1 < n_docs && (i1 == i0 || offsets.back() + pv.tok_cnt_host[docs[(size_t)i1]] <= slice); ++i1) {
                    const int64_t T = pv.tok_cnt_host[docs[(size_t)i1]], blk0 = pv.blk_off_host[docs[(size_t)i1]];
                    for (int64_t t = 0; t < T; t += kMsBlkRows)
                        blocks.push_back(ViewTokBlock{blk0 + t / kMsBlkRows, offsets.back() + t, (int32_t)std::min<int64_t>(kMsBlkRows, T - t), 0});
                    offsets.push_back(offsets.back() + T);
                }
            } catch (const std::bad_alloc&) {
                return fail(parent, MI355DR_E_NOMEM, "view_create: out of host memory for a slice's block table");
            }
            HIPCHECK(parent, blocks_dev.grow(blocks.size() * sizeof(ViewTokBlock)));
            HIPCHECK(parent, hipMemcpyAsync(blocks_dev.p, blocks.data(), blocks.size() * sizeof(ViewTokBlock), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_view_gather_toks, dim3((unsigned)blocks.size()), dim3(64 * kViewWaves), 0, s, pv.tok, blocks_dev.p, d,
                               pv.dpad, stage.p);
            HIPCHECK(parent, hipGetLastError());
            HIPCHECK(parent, hipStreamSynchronize(s));  // (also: `blocks` is pageable and is rewritten for the next slice)
            VIEWCHECK(parent, view, mi355dr_add_multivec_device(view, stage.p, offsets.data(), i1 - i0));
        }
        CHECK(view_upload_map(parent, docs, view->view_doc_map));
    }
    view->view_rows = n_rows;
    view->view_docs = n_docs;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_view_create(mi355dr_index* parent, const int64_t* row_ids, int64_t m_rows, const int64_t* doc_ids, int64_t m_docs,
                        mi355dr_index** out_view) {
    if (out_view) *out_view = nullptr;
    if (!parent) return fail(nullptr, MI355DR_E_INVALID, "null index");
    if (!out_view) return fail(parent, MI355DR_E_INVALID, "view_create: out_view is null");
    if (m_rows < 0 || m_docs < 0 || (m_rows > 0 && !row_ids) || (m_docs > 0 && !doc_ids))
        return fail(parent, MI355DR_E_INVALID, "view_create: counts must be >= 0 and a list with a count not null");
    std::lock_guard<std::mutex> g(parent->mu);
    if (parent->is_view) return view_refuses(parent, "view_create", /*ask_parent=*/true);
    HIPCHECK(parent, hipSetDevice(parent->device));
    CHECK(drain_pending(parent));
    mi355dr_index* view = nullptr;
    int rc = mi355dr_create(&view, parent->device, parent->dim, parent->metric);
    if (rc != MI355DR_OK) return fail(parent, rc, std::string("view_create: ") + mi355dr_last_error(nullptr));
    rc = view_build(parent, view, row_ids, m_rows, doc_ids, m_docs);
    if (rc != MI355DR_OK) {
        mi355dr_destroy(view);  // (everything the view allocated goes with it; the parent was only read)
        return rc;
    }
    view->is_view = true;  // from here on: read-only, and the id-taking entry points refer to the parent
    *out_view = view;
    return MI355DR_OK;
}

int64_t mi355dr_size(const mi355dr_index* idx) { return idx ? idx->n : -1; }
int64_t mi355dr_live_rows(const mi355dr_index* idx) { return idx ? idx->n - idx->dead_n : -1; }
int mi355dr_dim(const mi355dr_index* idx) { return idx ? idx->dim : -1; }

int mi355dr_get_rows(mi355dr_index* idx, int64_t row0, int64_t n, float* out) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (row0 < 0 || n < 0 || row0 + n > idx->n || (n > 0 && !out)) return fail(idx, MI355DR_E_INVALID, "bad row range");
    if (n == 0) return MI355DR_OK;
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipMemcpyAsync(out, idx->rows + row0 * idx->dim, (size_t)n * idx->dim * sizeof(float),
                                 hipMemcpyDeviceToHost, idx->stream));
    HIPCHECK(idx, hipStreamSynchronize(idx->stream));
    return MI355DR_OK;
}

int mi355dr_search(mi355dr_index* idx, const float* queries, int B, int k, double* out_dist, int64_t* out_rows) {
    Call c;
    CHECK(begin_call(idx, "search", nullptr, kCallDrain, c, [&] { return check_search_args(idx, queries, B, k, out_dist, out_rows); }));
    const CallIO<> io{/*host=*/true, c.s, queries, {out_dist, out_rows, nullptr}, k};
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const float* q = nullptr;
        CHECK(block_queries(idx, io, b0, nb, &q));
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        CHECK(search_block(idx, c.s, q, nb, k, o.dist, o.rows));
        CHECK(block_return(idx, io, b0, nb, o));
        HIPCHECK(idx, hipStreamSynchronize(c.s));
    }
    return MI355DR_OK;
}

static int search_device_async_locked(mi355dr_index* idx, const float* queries_dev, int B, int k, double* out_dist_dev,
                                      int64_t* out_rows_dev, hipStream_t s, int64_t* ticket) {
    // a block in flight on ANOTHER stream is finished first: the per-search state is shared and only stream order protects it
    if (idx->seq_done < idx->seq_next && idx->pend[(idx->seq_next - 1) % kPendingRing].stream != s) CHECK(drain_pending(idx));
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        if (idx->seq_next - idx->seq_done >= kPendingRing) CHECK(complete_until(idx, idx->seq_done + 1));  // the ring is full: finish the oldest block
        Pending& p = idx->pend[idx->seq_next % kPendingRing];
        CHECK(enqueue_block(idx, s, queries_dev + (int64_t)b0 * idx->dim, nb, k, out_dist_dev + (int64_t)b0 * k,
                            out_rows_dev + (int64_t)b0 * k, p));
        idx->seq_next++;
    }
    if (ticket) *ticket = idx->seq_next;  // every block below this sequence number belongs to (or precedes) this call
    return MI355DR_OK;
}

int mi355dr_search_device_async(mi355dr_index* idx, const float* queries_dev, int B, int k, double* out_dist_dev,
                                int64_t* out_rows_dev, void* stream, int64_t* ticket) {
    CHECK(check_search_args(idx, queries_dev, B, k, out_dist_dev, out_rows_dev));
    if (!ticket) return fail(idx, MI355DR_E_INVALID, "ticket is null");
    std::lock_guard<std::mutex> g(idx->mu);
    HIPCHECK(idx, hipSetDevice(idx->device));
    return search_device_async_locked(idx, queries_dev, B, k, out_dist_dev, out_rows_dev,
                                      stream ? (hipStream_t)stream : idx->stream, ticket);
}

int mi355dr_search_wait(mi355dr_index* idx, int64_t ticket) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (ticket < 0 || ticket > idx->seq_next) return fail(idx, MI355DR_E_INVALID, "unknown ticket");
    HIPCHECK(idx, hipSetDevice(idx->device));
    return complete_until(idx, ticket);
}

int mi355dr_search_device(mi355dr_index* idx, const float* queries_dev, int B, int k, double* out_dist_dev,
                          int64_t* out_rows_dev, void* stream) {
    CHECK(check_search_args(idx, queries_dev, B, k, out_dist_dev, out_rows_dev));
    std::lock_guard<std::mutex> g(idx->mu);
    HIPCHECK(idx, hipSetDevice(idx->device));
    int64_t ticket = 0;
    CHECK(search_device_async_locked(idx, queries_dev, B, k, out_dist_dev, out_rows_dev,
                                     stream ? (hipStream_t)stream : idx->stream, &ticket));
    return drain_pending(idx);
}

// ---- search within a listed subset of rows (DESIGN.md section 4.5 "Gathered scan") -------------------------------------
namespace {
// the caller's global ids -> idx->subset_ids (local rows, ascending, unique); *m_out = how many.  Nothing of the index or of
// the per-search state has been touched when this fails.
int subset_upload_ids(mi355dr_index* idx, hipStream_t s, const int64_t* row_ids, int64_t m, int64_t* m_out) {
    std::vector<int32_t> ids;
    try {
        subset_prepare_ids(row_ids, m, idx->row_offset, idx->n, ids);
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "search_subset: out of host memory for the row list");
    }
    *m_out = (int64_t)ids.size();
    if (ids.empty()) return MI355DR_OK;
    HIPCHECK(idx, idx->subset_ids.grow(ids.size() * sizeof(int32_t)));
    HIPCHECK(idx, hipMemcpyAsync(idx->subset_ids, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipStreamSynchronize(s));  // (`ids` is pageable and leaves with this frame)
    return MI355DR_OK;
}

// (for `host`, here and in the families below, see CallIO)
int search_subset_impl(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* row_ids, int64_t m,
                       double* out_dist, int64_t* out_rows, void* stream, bool host) {
    Call c;
    CHECK(begin_call(idx, "search_subset", stream, kCallNoView | kCallDrain, c, [&]() -> int {
        CHECK(check_search_args(idx, queries, B, k, out_dist, out_rows));
        if (m < 0 || (m > 0 && !row_ids)) return fail(idx, MI355DR_E_INVALID, "search_subset: m must be >= 0 and row_ids not null");
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    int64_t m_valid = 0;
    CHECK(subset_upload_ids(idx, c.s, row_ids, m, &m_valid));
    const CallIO<> io{host, c.s, queries, {out_dist, out_rows, nullptr}, k};
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const float* q = nullptr;
        CHECK(block_queries(idx, io, b0, nb, &q));
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        CHECK(subset_block(idx, c.s, q, nb, k, m_valid, o.dist, o.rows));  // (complete on return)
        CHECK(block_return(idx, io, b0, nb, o));
        if (host) HIPCHECK(idx, hipStreamSynchronize(c.s));
    }
    idx->s_subset_searches++;
    idx->s_subset_rows_scored += m_valid * B;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_search_subset(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* row_ids, int64_t m,
                          double* out_dist, int64_t* out_rows) {
    return search_subset_impl(idx, queries, B, k, row_ids, m, out_dist, out_rows, nullptr, /*host=*/true);
}

int mi355dr_search_subset_device(mi355dr_index* idx, const float* queries_dev, int B, int k, const int64_t* row_ids, int64_t m,
                                 double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return search_subset_impl(idx, queries_dev, B, k, row_ids, m, out_dist_dev, out_rows_dev, stream, /*host=*/false);
}

int mi355dr_score_subset(mi355dr_index* idx, const float* queries, int B, const int64_t* row_ids, int m, double* out_dist) {
    Call c;
    CHECK(begin_call(idx, "score_subset", nullptr, kCallNoView | kCallDrain, c, [&]() -> int {
        if (B < 0 || m < 0) return fail(idx, MI355DR_E_INVALID, "score_subset: B and m must be >= 0");
        if (B > 0 && (!queries || (m > 0 && (!row_ids || !out_dist)))) return fail(idx, MI355DR_E_INVALID, "null buffer");
        return MI355DR_OK;
    }));
    const int64_t total = (int64_t)B * m;
    for (int64_t i = 0; i < total; ++i) out_dist[i] = NAN;
    if (total == 0) return MI355DR_OK;
    std::vector<int32_t> pq;
    std::vector<int64_t> pr, where;  // where: the pair's slot in out_dist
    std::vector<double> got;
    PairBufs bufs;
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        try {  // pairs for the ids inside this index only: k_rescore_pairs does not range-check
            pq.clear();
            pr.clear();
            where.clear();
            for (int b = 0; b < nb; ++b)
                for (int j = 0; j < m; ++j) {
                    const int64_t at = (int64_t)(b0 + b) * m + j, r = subset_local_row(row_ids[at], idx->row_offset, idx->n);
                    if (r < 0) continue;
                    pq.push_back(b);
                    pr.push_back(r);
                    where.push_back(at);
                }
            got.resize(pq.size());
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "score_subset: out of host memory for the pair list");
        }
        const int64_t n_pairs = (int64_t)pq.size();
        if (n_pairs == 0) continue;
        CHECK(rescore_host_pairs(idx, bufs, queries + (int64_t)b0 * idx->dim, nb, pq.data(), pr.data(), n_pairs, nullptr, got.data()));
        for (int64_t i = 0; i < n_pairs; ++i) out_dist[where[i]] = got[i];  // (a removed row, an undefined distance: the kernel's NaN)
    }
    return MI355DR_OK;
}

// ---- MMR: diversity-aware top-k over a candidate list (csrc/k_mmr.h) -----------------------------
namespace {
int check_mmr_lambda(mi355dr_index* idx, const char* what, double lambda) {
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(idx, MI355DR_E_INVALID, std::string(what) + ": lambda must be in [0, 1]");
    return MI355DR_OK;
}

// nb lists [nb, stride] in idx->mmr.cand_* -> [nb, k] picks; asynchronous on the stream
int launch_mmr(mi355dr_index* idx, hipStream_t s, int nb, int stride, int k, double lambda, double* out_dist_dev,
               int64_t* out_rows_dev) {
    hipLaunchKernelGGL(k_mmr_select, dim3(nb), dim3(kMmrThreads), mmr_lds_bytes(idx->dim, stride), s, idx->mmr.cand_rows.p,
                       idx->mmr.cand_dist.p, stride, idx->rows.p, idx->nrm2.p, idx->n, idx->row_offset, idx->dim, idx->metric, k,
                       lambda, out_dist_dev, out_rows_dev, idx->mmr.pairs_dev.p);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// the call's last step (the stream is idle): the kernel's pair counter into the stats
int mmr_finish(mi355dr_index* idx, int B) {
    unsigned long long pairs = 0;
    HIPCHECK(idx, hipMemcpy(&pairs, idx->mmr.pairs_dev.p, sizeof(pairs), hipMemcpyDeviceToHost));
    idx->s_mmr_searches++;
    idx->s_mmr_queries += B;
    idx->s_mmr_pairs += (int64_t)pairs;
    return MI355DR_OK;
}

int search_mmr_impl(mi355dr_index* idx, const float* queries, int B, int k, int fetch_k, double lambda, double* out_dist,
                    int64_t* out_rows, void* stream, bool host) {
    Call c;
    CHECK(begin_call(idx, "search_mmr", stream, kCallNoView | kCallDrain, c, [&]() -> int {
        CHECK(check_search_args(idx, queries, B, k, out_dist, out_rows));
        CHECK(check_mmr_lambda(idx, "search_mmr", lambda));
        if (fetch_k < k) return fail(idx, MI355DR_E_INVALID, "search_mmr: fetch_k must be >= k");
        if (fetch_k > kMmrMax) return fail(idx, MI355DR_E_UNSUPPORTED, "search_mmr: fetch_k exceeds 1024");
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    HIPCHECK(idx, idx->mmr.reserve(std::min(B, kQBlockMax), fetch_k));
    HIPCHECK(idx, hipMemsetAsync(idx->mmr.pairs_dev.p, 0, sizeof(unsigned long long), c.s));
    const CallIO<> io{host, c.s, queries, {out_dist, out_rows, nullptr}, k};
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const float* q = nullptr;
        CHECK(block_queries(idx, io, b0, nb, &q));
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        // the ordinary search of the block at fetch_k (screened, fix-ups completed), then the selection behind it
        CHECK(search_block(idx, c.s, q, nb, fetch_k, idx->mmr.cand_dist.p, idx->mmr.cand_rows.p));
        CHECK(launch_mmr(idx, c.s, nb, fetch_k, k, lambda, o.dist, o.rows));
        CHECK(block_return(idx, io, b0, nb, o));
    }
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    return mmr_finish(idx, B);
}
}  // namespace

int mi355dr_search_mmr(mi355dr_index* idx, const float* queries, int B, int k, int fetch_k, double lambda, double* out_dist,
                       int64_t* out_rows) {
    return search_mmr_impl(idx, queries, B, k, fetch_k, lambda, out_dist, out_rows, nullptr, /*host=*/true);
}

int mi355dr_search_mmr_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int fetch_k, double lambda,
                              double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return search_mmr_impl(idx, queries_dev, B, k, fetch_k, lambda, out_dist_dev, out_rows_dev, stream, /*host=*/false);
}

int mi355dr_mmr_select(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* cand_rows, int m, double lambda,
                       double* out_dist, int64_t* out_rows) {
    Call c;
    CHECK(begin_call(idx, "mmr_select", nullptr, kCallNoView | kCallDrain, c, [&]() -> int {
        CHECK(check_search_args(idx, queries, B, k, out_dist, out_rows));
        CHECK(check_mmr_lambda(idx, "mmr_select", lambda));
        if (m < 0 || (B > 0 && m > 0 && !cand_rows)) return fail(idx, MI355DR_E_INVALID, "mmr_select: m must be >= 0 and cand_rows not null");
        if (m > kMmrMax) return fail(idx, MI355DR_E_UNSUPPORTED, "mmr_select: m exceeds 1024");
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    for (int64_t i = 0; i < (int64_t)B * k; ++i) {
        out_dist[i] = NAN;
        out_rows[i] = -1;
    }
    hipStream_t s = c.s;
    HIPCHECK(idx, idx->mmr.reserve(std::min(B, kQBlockMax), std::max(m, 1)));
    HIPCHECK(idx, hipMemsetAsync(idx->mmr.pairs_dev.p, 0, sizeof(unsigned long long), s));
    const CallIO<> io{/*host=*/true, s, nullptr, {out_dist, out_rows, nullptr}, k};  // (the queries go with the pairs)
    std::vector<int32_t> pq;
    std::vector<int64_t> pr, first, ordered_rows;  // first[b]: query b's first pair
    std::vector<double> got, ordered_dist;
    std::vector<MmrCand> list;
    PairBufs bufs;
    for (int b0 = 0; b0 < B && m > 0; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        try {  // every query's list: in-index rows, each once (k_rescore_pairs does not range-check)
            pr.clear();
            first.assign(1, 0);
            for (int b = 0; b < nb; ++b) {
                mmr_unique_rows(cand_rows + (int64_t)(b0 + b) * m, m, idx->row_offset, idx->n, pr);
                first.push_back((int64_t)pr.size());
            }
            pq.resize(pr.size());
            for (int b = 0; b < nb; ++b) std::fill(pq.begin() + first[b], pq.begin() + first[b + 1], b);
            got.resize(pr.size());
            ordered_dist.assign((size_t)nb * m, (double)NAN);
            ordered_rows.assign((size_t)nb * m, -1);
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "mmr_select: out of host memory for the candidate lists");
        }
        const int64_t n_pairs = (int64_t)pr.size();
        if (n_pairs == 0) continue;
        CHECK(rescore_host_pairs(idx, bufs, queries + (int64_t)b0 * idx->dim, nb, pq.data(), pr.data(), n_pairs, nullptr, got.data()));
        // each list into the total order: a removed row (the kernel's NaN) and a live row without a distance come last, behind
        // the eligible prefix k_mmr_select stops at
        try {
            for (int b = 0; b < nb; ++b) {
                list.clear();
                for (int64_t i = first[b]; i < first[b + 1]; ++i) list.push_back(MmrCand{got[i], pr[i]});
                mmr_order(list.data(), (int64_t)list.size());
                for (size_t j = 0; j < list.size(); ++j) {
                    ordered_dist[(size_t)b * m + j] = list[j].dist;
                    ordered_rows[(size_t)b * m + j] = list[j].row + idx->row_offset;
                }
            }
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "mmr_select: out of host memory for the candidate lists");
        }
        HIPCHECK(idx, hipMemcpyAsync(idx->mmr.cand_dist.p, ordered_dist.data(), (size_t)nb * m * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(idx->mmr.cand_rows.p, ordered_rows.data(), (size_t)nb * m * sizeof(int64_t), hipMemcpyHostToDevice, s));
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        CHECK(launch_mmr(idx, s, nb, m, k, lambda, o.dist, o.rows));
        CHECK(block_return(idx, io, b0, nb, o));
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the ordered lists are pageable and are rewritten for the next block)
    }
    HIPCHECK(idx, hipStreamSynchronize(s));
    return mmr_finish(idx, B);
}

// ---- grouped search: sub-query top-k lists fused into one per group (csrc/k_groups.h) -------------
namespace {
// the call's shape: S lists of `width` entries in G groups, k_out results per group.  *np_max: the padded size of the largest
// group (a power of two, >= 1).  Nothing has been touched when this fails.
int check_groups(mi355dr_index* idx, const char* what, int S, int width, const int32_t* offs, int G, int k_out, int* np_max) {
    const std::string w(what);
    if (G < 0 || S < 0) return fail(idx, MI355DR_E_INVALID, w + ": G and S must be >= 0");
    if (width <= 0 || k_out <= 0) return fail(idx, MI355DR_E_INVALID, w + ": the list width and k must be > 0");
    *np_max = 1;
    if (G == 0) {
        if (S != 0) return fail(idx, MI355DR_E_INVALID, w + ": group_offsets must end at S");
        return MI355DR_OK;
    }
    if (!offs) return fail(idx, MI355DR_E_INVALID, w + ": group_offsets is null");
    if (offs[0] != 0) return fail(idx, MI355DR_E_INVALID, w + ": group_offsets must start at 0");
    int64_t largest = 0;
    for (int g = 0; g < G; ++g) {
        if (offs[g + 1] < offs[g]) return fail(idx, MI355DR_E_INVALID, w + ": group_offsets must not decrease");
        largest = std::max(largest, (int64_t)(offs[g + 1] - offs[g]) * width);
    }
    if (offs[G] != S) return fail(idx, MI355DR_E_INVALID, w + ": group_offsets must end at S");
    if (k_out > kSortMax) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": k exceeds 4096");
    if (largest > kSortMax) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": a group holds more than 4096 entries");
    *np_max = groups_pow2(largest);
    return MI355DR_OK;
}

// the offsets into the handle's buffer, then ONE launch over all G groups; asynchronous on the stream (the caller waits:
// `offs` is pageable host memory)
int launch_groups(mi355dr_index* idx, hipStream_t s, const double* vals, const int64_t* rows, int width, const int32_t* offs,
                  int G, int np_max, int k_out, double* out_vals, int64_t* out_rows, int32_t* out_count) {
    HIPCHECK(idx, hipMemcpyAsync(idx->grp.offsets.p, offs, (size_t)(G + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_merge_groups, dim3(G), dim3(kGroupsThreads), groups_lds_bytes(np_max), s, vals, rows, width,
                       idx->grp.offsets.p, np_max, k_out, out_vals, out_rows, out_count);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

int search_groups_impl(mi355dr_index* idx, const float* queries, const int32_t* offs, int G, int k, int fetch_k, double* out_dist,
                       int64_t* out_rows, int32_t* out_count, void* stream, bool host) {
    int S = 0, np_max = 1;
    Call c;
    CHECK(begin_call(idx, "search_groups", stream, kCallDrain, c, [&]() -> int {
        if (G < 0 || k <= 0 || fetch_k <= 0) return fail(idx, MI355DR_E_INVALID, "search_groups: G must be >= 0, k and fetch_k > 0");
        if (G > 0 && !offs) return fail(idx, MI355DR_E_INVALID, "search_groups: group_offsets is null");
        S = G > 0 ? offs[G] : 0;
        if (G > 0 && (!out_dist || !out_rows || (S > 0 && !queries))) return fail(idx, MI355DR_E_INVALID, "search_groups: null buffer");
        if (fetch_k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "search_groups: fetch_k exceeds 1024");
        return check_groups(idx, "search_groups", S, fetch_k, offs, G, k, &np_max);
    }));
    if (G == 0) return MI355DR_OK;
    HIPCHECK(idx, idx->grp.reserve(G, std::max(S, 1), fetch_k, k, host));
    // the ordinary search of every sub-query at fetch_k (screened, fix-ups completed), block by block ...
    const CallIO<int32_t> io{host, c.s, queries, {out_dist, out_rows, out_count}, k};
    for (int b0 = 0; b0 < S; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, S - b0);
        const float* q = nullptr;
        CHECK(block_queries(idx, io, b0, nb, &q));
        CHECK(search_block(idx, c.s, q, nb, fetch_k, idx->grp.cand_dist.p + (int64_t)b0 * fetch_k,
                           idx->grp.cand_rows.p + (int64_t)b0 * fetch_k));
    }
    // ... then one merge behind all of them: a group may straddle two blocks.  The [G, k] results are one "block" of G lines
    const BlockOut<int32_t> o =
        host ? BlockOut<int32_t>{idx->grp.out_dist.p, idx->grp.out_rows.p, out_count ? idx->grp.count.p : nullptr} : io.out;
    CHECK(launch_groups(idx, c.s, idx->grp.cand_dist.p, idx->grp.cand_rows.p, fetch_k, offs, G, np_max, k, o.dist, o.rows, o.count));
    CHECK(block_return(idx, io, 0, G, o));
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    idx->s_group_searches++;
    idx->s_group_subqueries += S;
    idx->s_groups_merged += G;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_merge_groups_device(mi355dr_index* idx, const double* vals_dev, const int64_t* rows_dev, int S, int width,
                                const int32_t* group_offsets, int G, int k_out, double* out_vals_dev, int64_t* out_rows_dev,
                                int32_t* out_count_dev, void* stream) {
    int np_max = 1;
    Call c;
    CHECK(begin_call(idx, "merge_groups", stream, /*flags=*/0, c, [&]() -> int {  // (no drain: it touches no per-search state)
        CHECK(check_groups(idx, "merge_groups", S, width, group_offsets, G, k_out, &np_max));
        if (G > 0 && (!out_vals_dev || !out_rows_dev || (S > 0 && (!vals_dev || !rows_dev))))
            return fail(idx, MI355DR_E_INVALID, "merge_groups: null buffer");
        return MI355DR_OK;
    }));
    if (G == 0) return MI355DR_OK;
    HIPCHECK(idx, idx->grp.reserve(G, 0, 0, 0, /*host=*/false));
    CHECK(launch_groups(idx, c.s, vals_dev, rows_dev, width, group_offsets, G, np_max, k_out, out_vals_dev, out_rows_dev,
                        out_count_dev));
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    idx->s_groups_merged += G;
    return MI355DR_OK;
}

int mi355dr_search_groups(mi355dr_index* idx, const float* queries, const int32_t* group_offsets, int G, int k, int fetch_k,
                          double* out_dist, int64_t* out_rows, int32_t* out_count) {
    return search_groups_impl(idx, queries, group_offsets, G, k, fetch_k, out_dist, out_rows, out_count, nullptr, /*host=*/true);
}

int mi355dr_search_groups_device(mi355dr_index* idx, const float* queries_dev, const int32_t* group_offsets, int G, int k,
                                 int fetch_k, double* out_dist_dev, int64_t* out_rows_dev, int32_t* out_count_dev, void* stream) {
    return search_groups_impl(idx, queries_dev, group_offsets, G, k, fetch_k, out_dist_dev, out_rows_dev, out_count_dev,
                              stream, /*host=*/false);
}

// ---- hybrid fusion: two ranked lists per query fused into one (csrc/k_fuse.h) -----------------------
namespace {
struct FuseLists {  // one call's inputs and outputs, all on the device or all on the host
    const double* vals[2];
    const int64_t* ids[2];
    const int64_t* map[2];
    int64_t map_len[2];
    int w[2];
    double* out_vals;
    int64_t* out_ids;
    int32_t* out_count;
};

// the call's shape and options; fills everything of *a but the pointers.  Nothing has been touched when this fails.
int check_fuse(mi355dr_index* idx, const char* what, const FuseLists& io, int B, int k_out, const mi355dr_fuse_opts* o, FuseArgs* a) {
    const std::string w(what);
    if (B < 0) return fail(idx, MI355DR_E_INVALID, w + ": B must be >= 0");
    if (io.w[0] <= 0 || io.w[1] <= 0 || k_out <= 0) return fail(idx, MI355DR_E_INVALID, w + ": the list widths and k_out must be > 0");
    if (!o) return fail(idx, MI355DR_E_INVALID, w + ": opts is null");
    if (o->method < MI355DR_FUSE_RRF || o->method > MI355DR_FUSE_CC_DBSF) return fail(idx, MI355DR_E_INVALID, w + ": unknown method");
    for (const int mode : {o->mode_1, o->mode_2})
        if (mode < MI355DR_FUSE_ONE_MINUS || mode > MI355DR_FUSE_AS_IS) return fail(idx, MI355DR_E_INVALID, w + ": unknown score mode");
    a->absent = 0.0;
    if (o->method == MI355DR_FUSE_RRF) {
        const int64_t far = (int64_t)o->rrf_k + (int64_t)o->fetch_k + 1;
        if (o->rrf_k < 0 || far <= 0) return fail(idx, MI355DR_E_INVALID, w + ": rrf_k must be >= 0 and rrf_k + fetch_k + 1 > 0");
        a->absent = 1.0 / (double)far;
    } else {
        if (!std::isfinite(o->weight)) return fail(idx, MI355DR_E_INVALID, w + ": weight is not finite");
        if (o->method == MI355DR_FUSE_CC_TMM && (!std::isfinite(o->min_1) || !std::isfinite(o->min_2)))
            return fail(idx, MI355DR_E_INVALID, w + ": tmm needs two finite minima");
    }
    for (int l = 0; l < 2; ++l)
        if (io.map[l] && io.map_len[l] < 0) return fail(idx, MI355DR_E_INVALID, w + ": map_len must be >= 0");
    if (B > 0 && (!io.vals[0] || !io.ids[0] || !io.vals[1] || !io.ids[1] || !io.out_vals || !io.out_ids))
        return fail(idx, MI355DR_E_INVALID, w + ": null buffer");
    if (io.w[0] > kFuseWidthMax || io.w[1] > kFuseWidthMax) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": a list is wider than 1024");
    if (k_out > kFuseMax) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": k_out exceeds 2048");
    static_assert(MI355DR_FUSE_RRF == kFuseRrf && MI355DR_FUSE_CC_MM == kFuseMm && MI355DR_FUSE_CC_TMM == kFuseTmm &&
                      MI355DR_FUSE_CC_Z == kFuseZ && MI355DR_FUSE_CC_DBSF == kFuseDbsf && MI355DR_FUSE_ONE_MINUS == kFuseOneMinus &&
                      MI355DR_FUSE_NEGATE == kFuseNegate && MI355DR_FUSE_AS_IS == kFuseAsIs,
                  "k_fuse.h numbers the methods and modes as the header does");
    a->method = o->method;
    a->mode[0] = o->mode_1;
    a->mode[1] = o->mode_2;
    a->rrf_k = o->rrf_k;
    a->weight = o->weight;
    a->tmin[0] = o->min_1;
    a->tmin[1] = o->min_2;
    a->w[0] = io.w[0];
    a->w[1] = io.w[1];
    a->np = groups_pow2((int64_t)io.w[0] + io.w[1]);  // <= kFuseMax
    a->k_out = k_out;
    return MI355DR_OK;
}

// ONE launch over all B queries, `dev` being the lists on the device; asynchronous on the stream
int launch_fuse(mi355dr_index* idx, hipStream_t s, const FuseLists& dev, int B, FuseArgs a) {
    for (int l = 0; l < 2; ++l) {
        a.vals[l] = dev.vals[l];
        a.ids[l] = dev.ids[l];
        a.map[l] = dev.map[l];
        a.map_len[l] = dev.map[l] ? dev.map_len[l] : 0;
    }
    a.out_vals = dev.out_vals;
    a.out_ids = dev.out_ids;
    a.out_count = dev.out_count;
    hipLaunchKernelGGL(k_fuse_lists, dim3(B), dim3(kFuseThreads), fuse_lds_bytes(a.np), s, a);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

int fuse_impl(mi355dr_index* idx, const FuseLists& io, int B, int k_out, const mi355dr_fuse_opts* opts, void* stream, bool host) {
    FuseArgs a{};
    Call c;
    CHECK(begin_call(idx, "fuse_lists", stream, /*flags=*/0, c, [&]() -> int {  // (no drain: it touches no per-search state)
        return check_fuse(idx, "fuse_lists", io, B, k_out, opts, &a);
    }));
    if (B == 0) return MI355DR_OK;
    FuseLists dev = io;
    if (host) {
        FuseBufs& f = idx->fuse;
        const int64_t lens[2] = {io.map[0] ? io.map_len[0] : 0, io.map[1] ? io.map_len[1] : 0};
        HIPCHECK(idx, f.reserve(B, io.w, lens, k_out));
        for (int l = 0; l < 2; ++l) {
            const size_t n = (size_t)B * io.w[l];
            HIPCHECK(idx, hipMemcpyAsync(f.vals[l].p, io.vals[l], n * sizeof(double), hipMemcpyHostToDevice, c.s));
            HIPCHECK(idx, hipMemcpyAsync(f.ids[l].p, io.ids[l], n * sizeof(int64_t), hipMemcpyHostToDevice, c.s));
            if (lens[l] > 0)
                HIPCHECK(idx, hipMemcpyAsync(f.map[l].p, io.map[l], (size_t)lens[l] * sizeof(int64_t), hipMemcpyHostToDevice, c.s));
            dev.vals[l] = f.vals[l].p;
            dev.ids[l] = f.ids[l].p;
            // (a map of length 0 strikes every entry out: any non-null pointer says "a map is given")
            dev.map[l] = io.map[l] ? (lens[l] > 0 ? f.map[l].p : (const int64_t*)f.ids[l].p) : nullptr;
        }
        dev.out_vals = f.out_vals.p;
        dev.out_ids = f.out_ids.p;
        dev.out_count = io.out_count ? f.count.p : nullptr;
    }
    CHECK(launch_fuse(idx, c.s, dev, B, a));
    if (host) {
        const size_t n = (size_t)B * k_out;
        HIPCHECK(idx, hipMemcpyAsync(io.out_vals, dev.out_vals, n * sizeof(double), hipMemcpyDeviceToHost, c.s));
        HIPCHECK(idx, hipMemcpyAsync(io.out_ids, dev.out_ids, n * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (io.out_count)
            HIPCHECK(idx, hipMemcpyAsync(io.out_count, dev.out_count, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    }
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    idx->s_fuse_calls++;
    idx->s_fuse_queries += B;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_fuse_lists_device(mi355dr_index* idx, const double* vals1_dev, const int64_t* ids1_dev, int w1, const int64_t* map1_dev,
                              int64_t map1_len, const double* vals2_dev, const int64_t* ids2_dev, int w2, const int64_t* map2_dev,
                              int64_t map2_len, int B, int k_out, const mi355dr_fuse_opts* opts, double* out_vals_dev,
                              int64_t* out_ids_dev, int32_t* out_count_dev, void* stream) {
    const FuseLists io{{vals1_dev, vals2_dev}, {ids1_dev, ids2_dev}, {map1_dev, map2_dev}, {map1_len, map2_len}, {w1, w2},
                       out_vals_dev, out_ids_dev, out_count_dev};
    return fuse_impl(idx, io, B, k_out, opts, stream, /*host=*/false);
}

int mi355dr_fuse_lists(mi355dr_index* idx, const double* vals1, const int64_t* ids1, int w1, const int64_t* map1, int64_t map1_len,
                       const double* vals2, const int64_t* ids2, int w2, const int64_t* map2, int64_t map2_len, int B, int k_out,
                       const mi355dr_fuse_opts* opts, double* out_vals, int64_t* out_ids, int32_t* out_count) {
    const FuseLists io{{vals1, vals2}, {ids1, ids2}, {map1, map2}, {map1_len, map2_len}, {w1, w2}, out_vals, out_ids, out_count};
    return fuse_impl(idx, io, B, k_out, opts, nullptr, /*host=*/true);
}

// ---- source-capped lists and search: at most `cap` entries per source (csrc/k_collapse.h) ----------
namespace {
struct CollapseLists {  // one call's inputs and outputs, all on the device or all on the host
    const double* vals;
    const int64_t* ids;
    const int64_t* keys;
    int64_t keys_len;
    double* out_vals;
    int64_t* out_ids;
    int64_t* out_keys;
    int32_t* out_pos;
    int32_t* out_count;
    int32_t* out_entries;
};

// the key table's own rules, shared by the list and the search forms
int check_collapse_keys(mi355dr_index* idx, const std::string& w, const int64_t* keys, int64_t keys_len, int cap) {
    if (cap <= 0) return fail(idx, MI355DR_E_INVALID, w + ": cap must be > 0");
    if (keys_len < 0) return fail(idx, MI355DR_E_INVALID, w + ": keys_len must be >= 0");
    if (keys && keys_len == 0) return fail(idx, MI355DR_E_INVALID, w + ": a key table of length 0 (pass NULL for no keys)");
    if (!keys && keys_len > 0) return fail(idx, MI355DR_E_INVALID, w + ": keys is null");
    return MI355DR_OK;
}

// `n` lists [n, w] -> the lines `lines` names (null: line s for list s); asynchronous on the stream
int launch_collapse(mi355dr_index* idx, hipStream_t s, int n, int w, const int32_t* lines, const CollapseLists& dev, int cap,
                    int k_out) {
    const int np = collapse_pow2(w);
    hipLaunchKernelGGL(k_collapse_lists, dim3(n), dim3(kCollapseThreads), collapse_lds_bytes(np), s, (const uint64_t*)dev.vals,
                       dev.ids, w, np, lines, dev.keys, dev.keys ? dev.keys_len : 0, cap, k_out, (uint64_t*)dev.out_vals,
                       dev.out_ids, dev.out_keys, dev.out_pos, dev.out_count, dev.out_entries);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

int collapse_lists_impl(mi355dr_index* idx, const CollapseLists& io, int w, int B, int cap, int k_out, void* stream, bool host) {
    Call c;
    CHECK(begin_call(idx, "collapse_lists", stream, /*flags=*/0, c, [&]() -> int {  // (no drain: it touches no per-search state)
        const std::string what("collapse_lists");
        if (B < 0) return fail(idx, MI355DR_E_INVALID, what + ": B must be >= 0");
        if (w <= 0 || k_out <= 0) return fail(idx, MI355DR_E_INVALID, what + ": the list width and k_out must be > 0");
        CHECK(check_collapse_keys(idx, what, io.keys, io.keys_len, cap));
        if (B > 0 && (!io.vals || !io.ids || !io.out_vals || !io.out_ids)) return fail(idx, MI355DR_E_INVALID, what + ": null buffer");
        if (w > kSortMax) return fail(idx, MI355DR_E_UNSUPPORTED, what + ": a list is wider than 4096");
        if (k_out > kSortMax) return fail(idx, MI355DR_E_UNSUPPORTED, what + ": k_out exceeds 4096");
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    CollapseLists dev = io;
    if (host) {
        CollapseBufs& b = idx->clp;
        HIPCHECK(idx, b.reserve_lists(B, w, io.keys ? io.keys_len : 0, k_out));
        const size_t n = (size_t)B * w;
        HIPCHECK(idx, hipMemcpyAsync(b.vals.p, io.vals, n * sizeof(double), hipMemcpyHostToDevice, c.s));
        HIPCHECK(idx, hipMemcpyAsync(b.ids.p, io.ids, n * sizeof(int64_t), hipMemcpyHostToDevice, c.s));
        if (io.keys) HIPCHECK(idx, hipMemcpyAsync(b.keys.p, io.keys, (size_t)io.keys_len * sizeof(int64_t), hipMemcpyHostToDevice, c.s));
        dev = CollapseLists{b.vals.p, b.ids.p, io.keys ? b.keys.p : nullptr, io.keys_len, b.out_vals.p, b.out_ids.p,
                            io.out_keys ? b.out_keys.p : nullptr, io.out_pos ? b.out_pos.p : nullptr,
                            io.out_count ? b.count.p : nullptr, io.out_entries ? b.entries.p : nullptr};
    }
    CHECK(launch_collapse(idx, c.s, B, w, nullptr, dev, cap, k_out));
    if (host) {
        const size_t n = (size_t)B * k_out;
        HIPCHECK(idx, hipMemcpyAsync(io.out_vals, dev.out_vals, n * sizeof(double), hipMemcpyDeviceToHost, c.s));
        HIPCHECK(idx, hipMemcpyAsync(io.out_ids, dev.out_ids, n * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (io.out_keys) HIPCHECK(idx, hipMemcpyAsync(io.out_keys, dev.out_keys, n * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
        if (io.out_pos) HIPCHECK(idx, hipMemcpyAsync(io.out_pos, dev.out_pos, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (io.out_count)
            HIPCHECK(idx, hipMemcpyAsync(io.out_count, dev.out_count, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        if (io.out_entries)
            HIPCHECK(idx, hipMemcpyAsync(io.out_entries, dev.out_entries, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    }
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    idx->s_collapse_calls++;
    return MI355DR_OK;
}

// what one call of the search forms carries besides its inner search
struct CollapseSearch {
    const char* what;
    const float* queries;
    int B, k, cap;
    const int64_t* keys;
    int64_t keys_len;
    int fetch_k, max_fetch;
    double* out_dist;
    int64_t* out_rows;
    int64_t* out_keys;
    int32_t* out_count;
    int32_t* out_state;
    void* stream;
    bool host;
};

// Both search forms and the sharded one.  `topk(s, q_dev, n, w, od, orow)`: the ordinary search of n device queries at width w
// into [n, w] device lists, screened and with its fix-ups completed (search_block; shard_topk_block over a communicator).
// `more_checks`: the form's own argument rules, behind the common ones.  `reserve_inner(nb_max)`: whatever `topk` may need for
// ANY round of a block of nb_max queries -- up to nb_max lists of max_fetch entries -- taken before the first search, so that no
// later round allocates (over a communicator: no rank can fail an allocation between two collectives of a call).
// (std::function parameters, not a template: the entry points below stand inside the file's extern "C" block.)
using CollapseTopK = std::function<int(hipStream_t, const float*, int, int, double*, int64_t*)>;
int search_collapsed_impl(mi355dr_index* idx, const CollapseSearch& a, unsigned flags, const std::function<int()>& more_checks,
                          const std::function<int(int)>& reserve_inner, const CollapseTopK& topk) {
    Call c;
    CHECK(begin_call(idx, a.what, a.stream, flags, c, [&]() -> int {
        const std::string what(a.what);
        CHECK(check_search_args(idx, a.queries, a.B, a.k, a.out_dist, a.out_rows));
        CHECK(check_collapse_keys(idx, what, a.keys, a.keys_len, a.cap));
        if (a.fetch_k < a.k) return fail(idx, MI355DR_E_INVALID, what + ": fetch_k must be >= k");
        if (a.max_fetch < a.fetch_k) return fail(idx, MI355DR_E_INVALID, what + ": max_fetch must be >= fetch_k");
        if (a.max_fetch > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, what + ": max_fetch exceeds 1024");
        return more_checks();
    }));
    const int B = a.B, k = a.k;
    if (B == 0) return MI355DR_OK;
    CollapseBufs& cb = idx->clp;
    const int nb_max = std::min(B, kQBlockMax);
    HIPCHECK(idx, cb.reserve_search(nb_max, a.max_fetch, k, idx->dim, a.host && a.keys ? a.keys_len : 0, a.host));
    CHECK(reserve_inner(nb_max));
    std::vector<int32_t> kept, entries, count, state;
    CollapsePlan plan;
    try {
        kept.resize(nb_max);
        entries.resize(nb_max);
        count.resize(nb_max);
        state.resize(nb_max);
        plan.lines.reserve(nb_max);
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, std::string(a.what) + ": out of host memory for the schedule");
    }
    const int64_t* keys_dev = a.keys;
    if (a.host && a.keys) {
        HIPCHECK(idx, hipMemcpyAsync(cb.keys.p, a.keys, (size_t)a.keys_len * sizeof(int64_t), hipMemcpyHostToDevice, c.s));
        keys_dev = cb.keys.p;
    }
    int64_t researched = 0, truncated = 0;
    const CallIO<> io{a.host, c.s, a.queries, {a.out_dist, a.out_rows, nullptr}, k};
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        // the block's queries where they stay readable through every round: not block_queries' qdev, which the inner search's
        // fix-ups overwrite -- the host form keeps a copy of its own
        const float* q = a.queries + (int64_t)b0 * idx->dim;
        if (a.host) {
            HIPCHECK(idx, hipMemcpyAsync(cb.q_all.p, q, (size_t)nb * idx->dim * sizeof(float), hipMemcpyHostToDevice, c.s));
            q = cb.q_all.p;
        }
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        CollapseLists dev{cb.cand_dist.p, cb.cand_rows.p, keys_dev, a.keys_len, o.dist, o.rows, nullptr, nullptr, cb.kept.p, cb.entries.p};
        if (a.out_keys) dev.out_keys = a.host ? cb.out_keys.p : a.out_keys + (int64_t)b0 * k;
        plan.begin(nb, k, a.fetch_k, a.max_fetch);
        const float* q_round = q;
        const int32_t* lines = nullptr;
        for (int n = nb;;) {
            // the ordinary search of the round's queries at f, the cap over their lists, (kept, entries) back
            CHECK(topk(c.s, q_round, n, plan.f, cb.cand_dist.p, cb.cand_rows.p));
            CHECK(launch_collapse(idx, c.s, n, plan.f, lines, dev, a.cap, k));
            HIPCHECK(idx, hipMemcpyAsync(kept.data(), cb.kept.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
            HIPCHECK(idx, hipMemcpyAsync(entries.data(), cb.entries.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
            HIPCHECK(idx, hipStreamSynchronize(c.s));
            if (!plan.advance(kept.data(), entries.data())) break;
            // the unfinished queries, and only they, side by side for the next round; their lists write their own lines
            n = (int)plan.lines.size();
            HIPCHECK(idx, hipMemcpyAsync(cb.lines.p, plan.lines.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.s));
            hipLaunchKernelGGL(k_gather_queries, dim3(n), dim3(128), 0, c.s, q, (const int*)cb.lines.p, idx->dim, cb.q_sub.p);
            HIPCHECK(idx, hipGetLastError());
            HIPCHECK(idx, hipStreamSynchronize(c.s));  // `plan.lines` (pageable) was read by the copy
            q_round = cb.q_sub.p;
            lines = cb.lines.p;
        }
        researched += plan.researched;
        for (int i = 0; i < nb; ++i) {
            count[i] = collapse_count(kept[i], k);
            state[i] = collapse_state(kept[i], entries[i], k, a.max_fetch);
            truncated += state[i] & kCollapseTruncated ? 1 : 0;
        }
        // distances and rows as every host form returns them; the keys behind them; count and state are the host's own words
        CHECK(block_return(idx, io, b0, nb, o));
        if (a.host) {
            if (a.out_keys)
                HIPCHECK(idx, hipMemcpyAsync(a.out_keys + (int64_t)b0 * k, dev.out_keys, (size_t)nb * k * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
            if (a.out_count) memcpy(a.out_count + b0, count.data(), (size_t)nb * sizeof(int32_t));
            if (a.out_state) memcpy(a.out_state + b0, state.data(), (size_t)nb * sizeof(int32_t));
        } else {
            if (a.out_count) HIPCHECK(idx, hipMemcpyAsync(a.out_count + b0, count.data(), (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, c.s));
            if (a.out_state) HIPCHECK(idx, hipMemcpyAsync(a.out_state + b0, state.data(), (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, c.s));
        }
        HIPCHECK(idx, hipStreamSynchronize(c.s));  // (the next block reuses the staging, the lists and the host words)
    }
    idx->s_collapse_searches++;
    idx->s_collapse_queries += B;
    idx->s_collapse_researched += researched;
    idx->s_collapse_truncated += truncated;
    return MI355DR_OK;
}

int search_collapsed_local(mi355dr_index* idx, const CollapseSearch& a) {
    return search_collapsed_impl(idx, a, kCallDrain, [] { return MI355DR_OK; }, [](int) { return MI355DR_OK; },
                                 [&](hipStream_t s, const float* q, int n, int w, double* od, int64_t* orow) {
                                     return search_block(idx, s, q, n, w, od, orow);
                                 });
}
}  // namespace

int mi355dr_collapse_lists_device(mi355dr_index* idx, const double* vals_dev, const int64_t* ids_dev, int w, int B,
                                  const int64_t* keys_dev, int64_t keys_len, int cap, int k_out, double* out_vals_dev,
                                  int64_t* out_ids_dev, int64_t* out_keys_dev, int32_t* out_pos_dev, int32_t* out_count_dev,
                                  int32_t* out_entries_dev, void* stream) {
    const CollapseLists io{vals_dev, ids_dev, keys_dev, keys_len, out_vals_dev, out_ids_dev, out_keys_dev, out_pos_dev,
                           out_count_dev, out_entries_dev};
    return collapse_lists_impl(idx, io, w, B, cap, k_out, stream, /*host=*/false);
}

int mi355dr_collapse_lists(mi355dr_index* idx, const double* vals, const int64_t* ids, int w, int B, const int64_t* keys,
                           int64_t keys_len, int cap, int k_out, double* out_vals, int64_t* out_ids, int64_t* out_keys,
                           int32_t* out_pos, int32_t* out_count, int32_t* out_entries) {
    const CollapseLists io{vals, ids, keys, keys_len, out_vals, out_ids, out_keys, out_pos, out_count, out_entries};
    return collapse_lists_impl(idx, io, w, B, cap, k_out, nullptr, /*host=*/true);
}

int mi355dr_search_collapsed(mi355dr_index* idx, const float* queries, int B, int k, int cap, const int64_t* keys, int64_t keys_len,
                             int fetch_k, int max_fetch, double* out_dist, int64_t* out_rows, int64_t* out_keys,
                             int32_t* out_count, int32_t* out_state) {
    return search_collapsed_local(idx, CollapseSearch{"search_collapsed", queries, B, k, cap, keys, keys_len, fetch_k, max_fetch,
                                                      out_dist, out_rows, out_keys, out_count, out_state, nullptr, /*host=*/true});
}

int mi355dr_search_collapsed_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int cap, const int64_t* keys_dev,
                                    int64_t keys_len, int fetch_k, int max_fetch, double* out_dist_dev, int64_t* out_rows_dev,
                                    int64_t* out_keys_dev, int32_t* out_count_dev, int32_t* out_state_dev, void* stream) {
    return search_collapsed_local(idx, CollapseSearch{"search_collapsed_device", queries_dev, B, k, cap, keys_dev, keys_len, fetch_k,
                                                      max_fetch, out_dist_dev, out_rows_dev, out_keys_dev, out_count_dev,
                                                      out_state_dev, stream, /*host=*/false});
}

// ---- range search: every row within a distance, counted on the device (csrc/k_range.h) ------------
namespace {
struct RangeSpan {
    int64_t r0, r1;
};

// slots of a query's result buffer: the option, never below the call's max_results (<= kKMax <= kSortMax)
inline int range_slots_for(const mi355dr_index* idx, int m) { return std::max(idx->range_slots, m); }

// the handle's range buffers for a block of nb queries, R slots each, lists of m entries and a redo list of `pairs` pairs;
// registers k_range_collect's LDS once
int ensure_range(mi355dr_index* idx, int nb, int R, int m, int64_t pairs) {
    HIPCHECK(idx, idx->rng.reserve(nb, R, m, pairs, idx->dim));
    if (idx->rng.collect_lds == 0) {
        const size_t lds = range_collect_lds(idx->dim);
        if (lds > 160 * 1024) return fail(idx, MI355DR_E_UNSUPPORTED, "dim too large for the range kernels' LDS budget");
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_range_collect, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        idx->rng.collect_lds = (int)lds;
    }
    return MI355DR_OK;
}

RangeState range_state(const mi355dr_index* idx, int R, int64_t pairs) {
    RangeState rs{};
    rs.key = idx->rng.key;
    rs.row = idx->rng.row;
    rs.count = idx->rng.count;
    rs.rkey = idx->rng.rkey;
    rs.xfrom = idx->rng.xfrom;
    rs.redo = idx->rng.redo;
    rs.redo_cap = (int)pairs;
    rs.stat = idx->rng.stat;
    rs.flag = idx->rng.flag;
    rs.R = R;
    return rs;
}

// k_range_collect over the block's nq queries (qlist == nullptr: queries 0 .. nq-1) behind the launch that filled their lists
int launch_range_collect(mi355dr_index* idx, hipStream_t s, const Pass& ps, const RangeState& rs, int form, int nq,
                         const int* qlist, int span, int64_t row0) {
    RangeCollectArgs ca{};
    ca.rows = idx->rows;
    ca.nrm2 = idx->nrm2;
    ca.q = idx->qdev;
    ca.st = idx->st;
    ca.rs = rs;
    ca.cand_row = idx->cand_row;
    ca.cand_val = idx->cand_val;
    ca.qlist = qlist;
    ca.flag8 = form != kRangeFormExact && ps.i8 ? idx->flag8.p : nullptr;
    ca.cap = ps.cap;
    ca.d = idx->dim;
    ca.metric = idx->metric;
    ca.form = form;
    ca.span = span;
    ca.row0 = row0;
    ca.n_rows = idx->n;
    hipLaunchKernelGGL(k_range_collect, dim3(nq), dim3(kRangeThreads), range_collect_lds(idx->dim), s, ca);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// exact range scan of rows [r0, r1) for the queries in qlist_dev[0 .. nq_all): groups of kScanQ, the scan launches as they
// are (their fixed thresholds were preset by k_range_prep), each followed by the exact form of k_range_collect
int range_scan_span(mi355dr_index* idx, hipStream_t s, const Pass& ps, const RangeState& rs, int nq_all, int span, int64_t r0,
                    int64_t r1) {
    for (int off = 0; off < nq_all; off += kScanQ) {
        const int nq = std::min(kScanQ, nq_all - off);
        CHECK(launch_scan(idx, s, idx->qlist_dev + off, nq, ps.cap, r0, r1));
        CHECK(launch_range_collect(idx, s, ps, rs, kRangeFormExact, nq, idx->qlist_dev + off, span, r0));
    }
    return MI355DR_OK;
}

// one block of nb <= kQBlockMax device-resident queries -> device outputs [nb, m] / [nb], complete on return
int range_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int nb, const double* radius, int m, double* od,
                int64_t* orow, int64_t* ocount) {
    // a pass decided as at k = 1: the int8 screen wherever AUTO has it at all, and (no two-wave prune at that k, screening or
    // not) the lists at option "cand_cap".  It is no top-k pass: last_pass_k stands
    const Pass ps = decide_pass(idx, 1, 0, false, "screen path unavailable (too many irregular rows)");
    if (ps.refused) return fail(idx, MI355DR_E_UNSUPPORTED, ps.refused);
    const int cap = ps.cap;
    const bool i8 = ps.i8, use_screen = ps.screening;
    // the spans: chunks of option "range_chunk_rows" rows, whole 256-row tiles (a screen launch starts at a tile edge)
    const int64_t chunk = round_up(std::max<int64_t>(idx->range_chunk_rows, kT2), kT2);
    std::vector<RangeSpan> spans;
    for (int64_t r0 = 0; r0 < idx->n; r0 += chunk) spans.push_back(RangeSpan{r0, std::min(idx->n, r0 + chunk)});
    const int n_main = (int)spans.size();
    const int R = range_slots_for(idx, m);
    const int64_t pairs = (int64_t)nb * std::max(n_main, 1);
    CHECK(ensure_range(idx, nb, R, m, pairs));
    const RangeState rs = range_state(idx, R, pairs);
    if (q_dev != idx->qdev)
        HIPCHECK(idx, hipMemcpyAsync(idx->qdev, q_dev, (size_t)nb * idx->dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    CHECK(launch_prep(idx, s, nb, (int)round_up(nb, screen_tile(nb)), idx->metric, i8));
    HIPCHECK(idx, hipMemcpyAsync(idx->rng.radius.p, radius, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipMemsetAsync(idx->rng.redo.p, 0, 2 * sizeof(int), s));
    HIPCHECK(idx, hipMemsetAsync(idx->rng.stat.p, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_range_prep, dim3((nb + kRangeThreads - 1) / kRangeThreads), dim3(kRangeThreads), 0, s,
                       (const double*)idx->rng.radius.p, nb, idx->metric, use_screen ? 1 : 0, idx->st, rs);
    HIPCHECK(idx, hipGetLastError());
    std::vector<int> all(nb);
    for (int i = 0; i < nb; ++i) all[i] = i;
    if (use_screen) {
        for (int i = 0; i < n_main; ++i) {
            // k_screen_rq's common flush period: hits are rare under a fixed, tight threshold (a wave whose queue fills
            // faster still flushes on its own)
            CHECK(launch_screen(idx, s, i8, nb, spans[i].r0, spans[i].r1, cap, /*emit_mode=*/0, idx->screen_flush_sync ? 15 : -1));
            CHECK(launch_range_collect(idx, s, ps, rs, kRangeFormScreen, nb, nullptr, i, spans[i].r0));
        }
        // rows this screen cannot see (irregular; for int8 also loose), as a search pass feeds them: "no bound" candidates,
        // here in list-sized pieces with a collect step each, so that they cannot overflow a list
        const int side_n = i8 ? idx->irr8_n : idx->irr_n;
        const int32_t* side = i8 ? idx->irr8_rows.p : idx->irr_rows.p;
        for (int i0 = 0; i0 < side_n; i0 += cap) {
            hipLaunchKernelGGL(k_emit_irregular, dim3(nb), dim3(64), 0, s, side + i0, std::min(cap, side_n - i0), idx->st,
                               idx->cand_row, idx->cand_val, cap, 0);
            HIPCHECK(idx, hipGetLastError());
            CHECK(launch_range_collect(idx, s, ps, rs, kRangeFormSide, nb, nullptr, -1, 0));
        }
    } else if (n_main > 0) {
        HIPCHECK(idx, hipMemcpyAsync(idx->qlist_dev, all.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, s));
        for (int i = 0; i < n_main; ++i) CHECK(range_scan_span(idx, s, ps, rs, nb, i, spans[i].r0, spans[i].r1));
    }
    // ---- the recorded (query, span) pairs, on the exact path: a pair that came from the screen form runs its span whole; one
    // whose list overflowed under the exact scan runs it in pieces of `cap` rows, which cannot overflow
    for (int round = 0;; ++round) {
        int hdr[2] = {0, 0};
        HIPCHECK(idx, hipMemcpyAsync(hdr, idx->rng.redo.p, sizeof(hdr), hipMemcpyDeviceToHost, s));
        HIPCHECK(idx, hipStreamSynchronize(s));
        if (hdr[1] != 0) return fail(idx, MI355DR_E_INTERNAL, "range search: the redo list overflowed");
        if (hdr[0] == 0) break;
        if (round >= 3) return fail(idx, MI355DR_E_INTERNAL, "range search: a list-sized piece overflowed its list");
        std::vector<int> rec((size_t)2 * hdr[0]);
        HIPCHECK(idx, hipMemcpyAsync(rec.data(), idx->rng.redo.p + 2, rec.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHECK(idx, hipMemsetAsync(idx->rng.redo.p, 0, 2 * sizeof(int), s));
        HIPCHECK(idx, hipStreamSynchronize(s));
        std::vector<std::vector<int>> by_code((size_t)2 * spans.size());  // [2 * span + in_pieces]: the queries
        for (int i = 0; i < hdr[0]; ++i) {
            const int q = rec[2 * i], code = rec[2 * i + 1];
            if (q < 0 || q >= nb || code < 0 || code >= (int)by_code.size())
                return fail(idx, MI355DR_E_INTERNAL, "range search: a redo record out of range");
            by_code[code].push_back(q);
        }
        for (size_t code = 0; code < by_code.size(); ++code) {
            const std::vector<int>& qs = by_code[code];
            if (qs.empty()) continue;
            const RangeSpan sp = spans[code >> 1];
            HIPCHECK(idx, hipMemcpyAsync(idx->qlist_dev, qs.data(), qs.size() * sizeof(int), hipMemcpyHostToDevice, s));
            if (code & 1) {
                for (int64_t p = sp.r0; p < sp.r1; p += cap) {
                    spans.push_back(RangeSpan{p, std::min(sp.r1, p + cap)});
                    CHECK(range_scan_span(idx, s, ps, rs, (int)qs.size(), (int)spans.size() - 1, p, std::min(sp.r1, p + cap)));
                }
            } else {
                CHECK(range_scan_span(idx, s, ps, rs, (int)qs.size(), (int)(code >> 1), sp.r0, sp.r1));
            }
        }
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the query lists are pageable and leave with this round)
        idx->s_range_redo_chunks += hdr[0];
    }
    // ---- sort, write out, flag
    const int np_max = groups_pow2(R);
    hipLaunchKernelGGL(k_range_finish, dim3(nb), dim3(kRangeThreads), range_finish_lds(np_max), s, rs, np_max, m, idx->row_offset,
                       (const int64_t*)idx->view_row_map.p, od, orow, ocount);
    HIPCHECK(idx, hipGetLastError());
    std::vector<int> flag(nb);
    std::vector<int64_t> counts(nb);
    unsigned long long st2[2] = {0, 0};
    HIPCHECK(idx, hipMemcpyAsync(flag.data(), idx->rng.flag.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(counts.data(), ocount, (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(st2, idx->rng.stat.p, sizeof(st2), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    for (int i = 0; i < nb; ++i) idx->s_range_in_range += counts[i];
    idx->s_range_candidates += (int64_t)st2[0];
    idx->s_range_rescored += (int64_t)st2[1];
    // ---- more rows in range than the buffer holds: the list is the ordinary top-max_results (all of it is in range); the
    // device count stands
    std::vector<int> fb;
    for (int i = 0; i < nb; ++i)
        if (flag[i]) fb.push_back(i);
    if (!fb.empty()) {
        const int nf = (int)fb.size();
        HIPCHECK(idx, hipMemcpyAsync(idx->rng.fb_map.p, fb.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_gather_queries, dim3(nf), dim3(128), 0, s, (const float*)idx->qdev.p, (const int*)idx->rng.fb_map.p,
                           idx->dim, idx->rng.fb_q.p);
        HIPCHECK(idx, hipGetLastError());
        HIPCHECK(idx, hipStreamSynchronize(s));  // `fb` (pageable) was read by the copy
        const int k_before = idx->last_pass_k;  // (the list of a range search: not the caller's most recent k)
        CHECK(search_block(idx, s, idx->rng.fb_q.p, nf, m, idx->rng.fb_dist.p, idx->rng.fb_rows.p));
        idx->last_pass_k = k_before;
        hipLaunchKernelGGL(k_scatter_results, dim3(nf), dim3(128), 0, s, (const double*)idx->rng.fb_dist.p,
                           (const int64_t*)idx->rng.fb_rows.p, (const int*)idx->rng.fb_map.p, m, od, orow);
        HIPCHECK(idx, hipGetLastError());
        HIPCHECK(idx, hipStreamSynchronize(s));
        idx->s_range_fallback_queries += nf;
    }
    return MI355DR_OK;
}

int search_range_impl(mi355dr_index* idx, const float* queries, int B, const double* radius, int m, double* out_dist,
                      int64_t* out_rows, int64_t* out_count, void* stream, bool host) {
    Call c;
    CHECK(begin_call(idx, "search_range", stream, kCallDrain, c, [&]() -> int {
        if (B <= 0 || m < 1) return fail(idx, MI355DR_E_INVALID, "search_range: B and max_results must be >= 1");
        if (m > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "search_range: max_results exceeds 1024");
        if (!queries || !radius || !out_dist || !out_rows || !out_count) return fail(idx, MI355DR_E_INVALID, "search_range: null buffer");
        return check_radii(idx, "search_range", radius, B);
    }));
    const CallIO<> io{host, c.s, queries, {out_dist, out_rows, out_count}, m};
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const float* q = nullptr;
        CHECK(block_queries(idx, io, b0, nb, &q));
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        CHECK(range_block(idx, c.s, q, nb, radius + b0, m, o.dist, o.rows, o.count));  // (complete on return)
        CHECK(block_return(idx, io, b0, nb, o));
        if (host) HIPCHECK(idx, hipStreamSynchronize(c.s));
    }
    idx->s_range_searches++;
    idx->s_range_queries += B;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_search_range(mi355dr_index* idx, const float* queries, int B, const double* radius, int max_results, double* out_dist,
                         int64_t* out_rows, int64_t* out_count) {
    return search_range_impl(idx, queries, B, radius, max_results, out_dist, out_rows, out_count, nullptr, /*host=*/true);
}

int mi355dr_search_range_device(mi355dr_index* idx, const float* queries_dev, int B, const double* radius, int max_results,
                                double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_count_dev, void* stream) {
    return search_range_impl(idx, queries_dev, B, radius, max_results, out_dist_dev, out_rows_dev, out_count_dev,
                             stream, /*host=*/false);
}

// ---- search by stored row: neighbours of rows, self excluded (csrc/k_rows.h) ---------------------
namespace {
// both families.  radius == nullptr: the top-k form (kout = k); else the range form (kout = max_results, out_count used).
// (the outputs' `host`: see CallIO; the ids are host memory in both forms)
int search_rows_impl(mi355dr_index* idx, const char* what, const int64_t* row_ids, int B, const double* radius, bool range,
                     int kout, int flags, double* out_dist, int64_t* out_rows, int64_t* out_count, void* stream, bool host) {
    const bool include_self = (flags & MI355DR_ROWS_INCLUDE_SELF) != 0;
    const int stride = kout + (include_self ? 0 : 1);  // the inner pass's list: room for the row itself
    Call c;
    CHECK(begin_call(idx, what, stream, kCallNoView | kCallDrain, c, [&]() -> int {
        const std::string w(what);
        if (B < 0) return fail(idx, MI355DR_E_INVALID, w + ": B must be >= 0");
        if (kout < 1) return fail(idx, MI355DR_E_INVALID, w + (range ? ": max_results must be >= 1" : ": k must be > 0"));
        if (flags & ~MI355DR_ROWS_INCLUDE_SELF) return fail(idx, MI355DR_E_INVALID, w + ": unknown flag bits");
        if (B > 0 && (!row_ids || !out_dist || !out_rows || (range && (!radius || !out_count))))
            return fail(idx, MI355DR_E_INVALID, w + ": null buffer");
        if (range) CHECK(check_radii(idx, w, radius, B));
        if (stride > kKMax)
            return fail(idx, MI355DR_E_UNSUPPORTED, w + (range ? ": max_results" : ": k") + (include_self ? "" : " + 1 (the row itself)") + " exceeds 1024");
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    hipStream_t s = c.s;
    HIPCHECK(idx, idx->rowq.reserve(std::min(B, kQBlockMax), stride, idx->dim, range));
    HIPCHECK(idx, hipMemsetAsync(idx->rowq.skipped_dev.p, 0, sizeof(unsigned long long), s));
    const CallIO<> io{host, s, nullptr, {out_dist, out_rows, out_count}, kout};  // (the queries are gathered rows; top-k form: no count)
    std::vector<double> rad;
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        HIPCHECK(idx, hipMemcpyAsync(idx->rowq.ids.p, row_ids + b0, (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_rows_gather, dim3(nb), dim3(kRowsThreads), 0, s, (const int64_t*)idx->rowq.ids.p, idx->row_offset,
                           idx->n, (const float*)idx->rows.p, (const float*)idx->nrm2.p, idx->dim, idx->rowq.q.p,
                           idx->rowq.valid.p, idx->rowq.pair_q.p, idx->rowq.pair_row.p, idx->rowq.skipped_dev.p);
        HIPCHECK(idx, hipGetLastError());
        if (idx->n > 0 && !range) {
            // the ordinary search of the gathered block (screened, fix-ups completed)
            CHECK(search_block(idx, s, idx->rowq.q.p, nb, stride, idx->rowq.cand_dist.p, idx->rowq.cand_rows.p));
        } else if (idx->n > 0) {
            // an id outside the shard asks for nothing (its slot is blanked below): no row is within -inf
            rad.assign(radius + b0, radius + b0 + nb);
            for (int b = 0; b < nb; ++b)
                if (subset_local_row(row_ids[b0 + b], idx->row_offset, idx->n) < 0) rad[b] = -INFINITY;
            HIPCHECK(idx, hipMemcpyAsync(idx->rowq.radius.p, rad.data(), (size_t)nb * sizeof(double), hipMemcpyHostToDevice, s));
            // every slot's distance to its own row, from the block's prepared queries: the bits a search returns for the pair
            HIPCHECK(idx, hipMemcpyAsync(idx->qdev, idx->rowq.q.p, (size_t)nb * idx->dim * sizeof(float), hipMemcpyDeviceToDevice, s));
            // (the int8 flag does not matter: the re-score reads st.qn alone, and range_block prepares the block again)
            CHECK(launch_prep(idx, s, nb, (int)round_up(nb, screen_tile(nb)), idx->metric, idle_i8(idx)));
            CHECK(launch_rescore(idx, s, idx->rowq.pair_q.p, idx->rowq.pair_row.p, nb, idx->rowq.self_dot.p, idx->rowq.self_dist.p));
            // the range pass of the gathered block (it prepares the block again; complete on return, `rad` has been read)
            CHECK(range_block(idx, s, idx->rowq.q.p, nb, rad.data(), stride, idx->rowq.cand_dist.p, idx->rowq.cand_rows.p,
                              idx->rowq.cand_count.p));
        }
        // (an empty index: every slot is invalid and the lists are not read)
        hipLaunchKernelGGL(k_rows_drop, dim3(nb), dim3(kRowsThreads), 0, s, (const double*)idx->rowq.cand_dist.p,
                           (const int64_t*)idx->rowq.cand_rows.p, stride, (const int64_t*)idx->rowq.ids.p,
                           (const int*)idx->rowq.valid.p, kout, include_self ? 1 : 0,
                           range ? (const int64_t*)idx->rowq.cand_count.p : nullptr, (const double*)idx->rowq.self_dist.p,
                           (const double*)idx->rowq.radius.p, o.dist, o.rows, o.count);
        HIPCHECK(idx, hipGetLastError());
        CHECK(block_return(idx, io, b0, nb, o));
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the next block reuses the id, query and list buffers)
    }
    unsigned long long skipped = 0;
    HIPCHECK(idx, hipMemcpy(&skipped, idx->rowq.skipped_dev.p, sizeof(skipped), hipMemcpyDeviceToHost));
    idx->s_rows_searches++;
    idx->s_rows_queries += B;
    idx->s_rows_skipped += (int64_t)skipped;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_search_rows(mi355dr_index* idx, const int64_t* row_ids, int B, int k, int flags, double* out_dist, int64_t* out_rows) {
    return search_rows_impl(idx, "search_rows", row_ids, B, nullptr, false, k, flags, out_dist, out_rows, nullptr, nullptr, /*host=*/true);
}

int mi355dr_search_rows_device(mi355dr_index* idx, const int64_t* row_ids, int B, int k, int flags, double* out_dist_dev,
                               int64_t* out_rows_dev, void* stream) {
    return search_rows_impl(idx, "search_rows", row_ids, B, nullptr, false, k, flags, out_dist_dev, out_rows_dev, nullptr,
                            stream, /*host=*/false);
}

int mi355dr_search_range_rows(mi355dr_index* idx, const int64_t* row_ids, int B, const double* radius, int max_results, int flags,
                              double* out_dist, int64_t* out_rows, int64_t* out_count) {
    return search_rows_impl(idx, "search_range_rows", row_ids, B, radius, true, max_results, flags, out_dist, out_rows, out_count,
                            nullptr, /*host=*/true);
}

int mi355dr_search_range_rows_device(mi355dr_index* idx, const int64_t* row_ids, int B, const double* radius, int max_results,
                                     int flags, double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_count_dev, void* stream) {
    return search_rows_impl(idx, "search_range_rows", row_ids, B, radius, true, max_results, flags, out_dist_dev, out_rows_dev,
                            out_count_dev, stream, /*host=*/false);
}

// ---- search by examples / Rocchio feedback: queries built on the device (csrc/k_combine.h) ---------
namespace {
enum ExamplesForm { kExCombine, kExSearch, kExFeedback };
struct ExamplesArgs {
    const char* what;
    ExamplesForm form;
    const float* queries;  // the base vectors [B, dim] or null (feedback: the queries)
    int B;
    const int64_t* pos_ids;  // HOST [B, mp]
    int mp;
    const int64_t* neg_ids;  // HOST [B, mn]
    int mn;
    double alpha, beta, gamma;
    int k, fb_k, flags;
    float* out_vectors;  // kExCombine: [B, dim]
    int32_t* out_valid;  // kExCombine: [B]
    double* out_dist;    // the searches: [B, k]
    int64_t* out_rows;
    void* stream;
    bool host;
};

inline bool weight_ok(double w) { return std::isfinite(w) && w >= 0.0; }

int launch_combine(mi355dr_index* idx, hipStream_t s, const float* q, int nb, const int64_t* pos, int mp, const int64_t* neg,
                   int mn, const double* pos_dist, const ExamplesArgs& a, float* q_out, int* valid) {
    hipLaunchKernelGGL(k_combine_rows, dim3(nb), dim3(kCombineThreads), 0, s, q, pos, mp, neg, mn, pos_dist, idx->row_offset,
                       idx->n, (const float*)idx->rows.p, (const float*)idx->nrm2.p, idx->dim, idx->metric, a.alpha, a.beta,
                       a.gamma, q_out, valid, idx->exq.counters.p);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

int launch_strike(mi355dr_index* idx, hipStream_t s, int nb, int stride, int mp, int mn, bool strike, int k, double* od,
                  int64_t* orow) {
    hipLaunchKernelGGL(k_examples_strike, dim3(nb), dim3(kCombineThreads), 0, s, (const double*)idx->exq.cand_dist.p,
                       (const int64_t*)idx->exq.cand_rows.p, stride, (const int64_t*)idx->exq.pos.p, mp,
                       (const int64_t*)idx->exq.neg.p, mn, strike ? 1 : 0, (const int*)idx->exq.valid.p, idx->n > 0 ? 0 : 1, k,
                       od, orow);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

int examples_impl(mi355dr_index* idx, const ExamplesArgs& a) {
    const bool keep = (a.flags & MI355DR_EXAMPLES_KEEP) != 0;
    const bool strike = a.form == kExSearch && !keep;
    const int B = a.B, d = idx ? idx->dim : 0;
    // the width of the inner pass's lists: room for every listed row (feedback: both passes share the lists)
    const int64_t stride = a.form == kExSearch ? (int64_t)a.k + (strike ? (int64_t)a.mp + a.mn : 0)
                                               : a.form == kExFeedback ? std::max(a.k, a.fb_k) : 0;
    Call c;
    CHECK(begin_call(idx, a.what, a.stream, kCallNoView | kCallDrain, c, [&]() -> int {
        const std::string w(a.what);
        if (B < 0) return fail(idx, MI355DR_E_INVALID, w + ": B must be >= 0");
        if (a.mp < 0 || a.mn < 0) return fail(idx, MI355DR_E_INVALID, w + ": mp and mn must be >= 0");
        if (a.form != kExCombine && a.k <= 0) return fail(idx, MI355DR_E_INVALID, w + ": k must be > 0");
        if (a.form == kExFeedback && a.fb_k <= 0) return fail(idx, MI355DR_E_INVALID, w + ": fb_k must be > 0");
        if (!weight_ok(a.alpha) || !weight_ok(a.beta) || !weight_ok(a.gamma))
            return fail(idx, MI355DR_E_INVALID, w + ": alpha, beta and gamma must be finite and >= 0");
        if (a.flags & ~MI355DR_EXAMPLES_KEEP) return fail(idx, MI355DR_E_INVALID, w + ": unknown flag bits");
        if (a.form != kExFeedback && !a.queries && a.mp == 0)
            return fail(idx, MI355DR_E_INVALID, w + ": neither a base vector nor a positive example");
        if (B > 0) {
            const bool outs = a.form == kExCombine ? a.out_vectors && a.out_valid : a.out_dist && a.out_rows;
            if (!outs || (a.mp > 0 && !a.pos_ids) || (a.mn > 0 && !a.neg_ids) || (a.form == kExFeedback && !a.queries))
                return fail(idx, MI355DR_E_INVALID, w + ": null buffer");
        }
        if (a.form == kExFeedback) {
            if (a.fb_k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": fb_k exceeds 1024");
            if (a.k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": k exceeds 1024");
        } else {
            if ((int64_t)a.mp + a.mn > kCombineMaxExamples) return fail(idx, MI355DR_E_UNSUPPORTED, w + ": mp + mn exceeds 1024");
            if (stride > kKMax)
                return fail(idx, MI355DR_E_UNSUPPORTED, w + (strike ? ": k + mp + mn (room for every listed row)" : ": k") + " exceeds 1024");
        }
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    hipStream_t s = c.s;
    const int nb_max = std::min(B, kQBlockMax);
    const int mp = a.form == kExFeedback ? a.fb_k : a.mp, mn = a.form == kExFeedback ? 0 : a.mn;
    const bool own_base = a.form == kExFeedback && a.host;
    // (every allocation before any work; the feedback form's positives are pass 1's own rows: no id buffer)
    HIPCHECK(idx, idx->exq.reserve(nb_max, a.form == kExFeedback ? 0 : mp, mn, (size_t)stride, d, own_base));
    HIPCHECK(idx, hipMemsetAsync(idx->exq.counters.p, 0, 2 * sizeof(unsigned long long), s));
    const CallIO<> io{a.host, s, a.queries, {a.out_dist, a.out_rows, nullptr}, a.k};
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const float* q = nullptr;
        if (a.queries) CHECK(block_queries(idx, io, b0, nb, &q));
        if (a.form != kExFeedback) {
            // (the ids are pageable: HIP stages such a copy before the call returns, as for the id lists of mutate_rows_impl)
            if (mp > 0)
                HIPCHECK(idx, hipMemcpyAsync(idx->exq.pos.p, a.pos_ids + (int64_t)b0 * mp, (size_t)nb * mp * sizeof(int64_t), hipMemcpyHostToDevice, s));
            if (mn > 0)
                HIPCHECK(idx, hipMemcpyAsync(idx->exq.neg.p, a.neg_ids + (int64_t)b0 * mn, (size_t)nb * mn * sizeof(int64_t), hipMemcpyHostToDevice, s));
        }
        if (a.form == kExCombine) {
            float* qv = a.host ? idx->exq.q.p : a.out_vectors + (int64_t)b0 * d;
            int* vv = a.host ? idx->exq.valid.p : (int*)a.out_valid + b0;
            CHECK(launch_combine(idx, s, q, nb, idx->exq.pos.p, mp, idx->exq.neg.p, mn, nullptr, a, qv, vv));
            if (a.host) {
                HIPCHECK(idx, hipMemcpyAsync(a.out_vectors + (int64_t)b0 * d, qv, (size_t)nb * d * sizeof(float), hipMemcpyDeviceToHost, s));
                HIPCHECK(idx, hipMemcpyAsync(a.out_valid + b0, vv, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
            }
            HIPCHECK(idx, hipStreamSynchronize(s));  // (the next block reuses the id and query buffers)
            continue;
        }
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        if (a.form == kExSearch) {
            CHECK(launch_combine(idx, s, q, nb, idx->exq.pos.p, mp, idx->exq.neg.p, mn, nullptr, a, idx->exq.q.p, idx->exq.valid.p));
            // the ordinary search of the combined block (screened, fix-ups completed); an empty index: the lists are not read
            if (idx->n > 0) CHECK(search_block(idx, s, idx->exq.q.p, nb, (int)stride, idx->exq.cand_dist.p, idx->exq.cand_rows.p));
            CHECK(launch_strike(idx, s, nb, (int)stride, mp, mn, strike, a.k, o.dist, o.rows));
        } else {
            if (own_base) {  // (a fix-up of pass 1 overwrites qdev, where block_queries staged the block)
                HIPCHECK(idx, hipMemcpyAsync(idx->exq.base.p, q, (size_t)nb * d * sizeof(float), hipMemcpyDeviceToDevice, s));
                q = idx->exq.base.p;
            }
            if (idx->n > 0) {
                // pass 1 at fb_k; its lists are the positives, read where they lie
                CHECK(search_block(idx, s, q, nb, a.fb_k, idx->exq.cand_dist.p, idx->exq.cand_rows.p));
            } else {
                HIPCHECK(idx, hipMemsetAsync(idx->exq.cand_rows.p, 0xFF, (size_t)nb * a.fb_k * sizeof(int64_t), s));  // (-1: no positives)
                HIPCHECK(idx, hipMemsetAsync(idx->exq.cand_dist.p, 0xFF, (size_t)nb * a.fb_k * sizeof(double), s));   // (NaN)
            }
            CHECK(launch_combine(idx, s, q, nb, idx->exq.cand_rows.p, a.fb_k, nullptr, 0, idx->exq.cand_dist.p, a, idx->exq.q.p,
                                 idx->exq.valid.p));
            // pass 2 at k over the same lists (the combination has been read: stream order), nothing struck
            if (idx->n > 0) CHECK(search_block(idx, s, idx->exq.q.p, nb, a.k, idx->exq.cand_dist.p, idx->exq.cand_rows.p));
            CHECK(launch_strike(idx, s, nb, a.k, 0, 0, false, a.k, o.dist, o.rows));
        }
        CHECK(block_return(idx, io, b0, nb, o));
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the next block reuses the id, query and list buffers)
    }
    unsigned long long counters[2] = {0, 0};
    HIPCHECK(idx, hipMemcpy(counters, idx->exq.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
    idx->s_examples_searches++;
    idx->s_examples_queries += B;
    idx->s_examples_skipped += (int64_t)counters[0];
    idx->s_examples_skipped_slots += (int64_t)counters[1];
    if (a.form == kExFeedback) idx->s_feedback_searches++;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_combine_rows(mi355dr_index* idx, const float* queries, int B, const int64_t* pos_ids, int mp, const int64_t* neg_ids,
                         int mn, double alpha, double beta, double gamma, float* out_vectors, int32_t* out_valid) {
    return examples_impl(idx, ExamplesArgs{"combine_rows", kExCombine, queries, B, pos_ids, mp, neg_ids, mn, alpha, beta, gamma, 0, 0,
                                           0, out_vectors, out_valid, nullptr, nullptr, nullptr, /*host=*/true});
}

int mi355dr_combine_rows_device(mi355dr_index* idx, const float* queries_dev, int B, const int64_t* pos_ids, int mp,
                                const int64_t* neg_ids, int mn, double alpha, double beta, double gamma, float* out_vectors_dev,
                                int32_t* out_valid_dev, void* stream) {
    return examples_impl(idx, ExamplesArgs{"combine_rows", kExCombine, queries_dev, B, pos_ids, mp, neg_ids, mn, alpha, beta, gamma,
                                           0, 0, 0, out_vectors_dev, out_valid_dev, nullptr, nullptr, stream, /*host=*/false});
}

int mi355dr_search_examples(mi355dr_index* idx, const float* queries, int B, const int64_t* pos_ids, int mp, const int64_t* neg_ids,
                            int mn, double alpha, double beta, double gamma, int k, int flags, double* out_dist,
                            int64_t* out_rows) {
    return examples_impl(idx, ExamplesArgs{"search_examples", kExSearch, queries, B, pos_ids, mp, neg_ids, mn, alpha, beta, gamma, k,
                                           0, flags, nullptr, nullptr, out_dist, out_rows, nullptr, /*host=*/true});
}

int mi355dr_search_examples_device(mi355dr_index* idx, const float* queries_dev, int B, const int64_t* pos_ids, int mp,
                                   const int64_t* neg_ids, int mn, double alpha, double beta, double gamma, int k, int flags,
                                   double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return examples_impl(idx, ExamplesArgs{"search_examples", kExSearch, queries_dev, B, pos_ids, mp, neg_ids, mn, alpha, beta,
                                           gamma, k, 0, flags, nullptr, nullptr, out_dist_dev, out_rows_dev, stream, /*host=*/false});
}

int mi355dr_search_feedback(mi355dr_index* idx, const float* queries, int B, int k, int fb_k, double alpha, double beta,
                            double* out_dist, int64_t* out_rows) {
    return examples_impl(idx, ExamplesArgs{"search_feedback", kExFeedback, queries, B, nullptr, 0, nullptr, 0, alpha, beta, 0.0, k,
                                           fb_k, 0, nullptr, nullptr, out_dist, out_rows, nullptr, /*host=*/true});
}

int mi355dr_search_feedback_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int fb_k, double alpha, double beta,
                                   double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return examples_impl(idx, ExamplesArgs{"search_feedback", kExFeedback, queries_dev, B, nullptr, 0, nullptr, 0, alpha, beta, 0.0,
                                           k, fb_k, 0, nullptr, nullptr, out_dist_dev, out_rows_dev, stream, /*host=*/false});
}

// ---- the derived searches over a row-sharded index (csrc/k_shard.h) ---------------------------------
// One frame (begin_call) per call, so nothing below may call a public entry point: the inner "sharded block at width w" is
// search_block straight into the packed planes, comm_all_gather, launch_merge with the rank stride.  Every rank enters every
// collective of a call in the same order, an empty shard included (it contributes empty lists, zero counts, invalid slots).
namespace {
int check_comm(mi355dr_index* idx) {
    if (!idx->comm && !idx->comm_custom) return fail(idx, MI355DR_E_INVALID, "mi355dr_comm_init has not been called on this index");
    return MI355DR_OK;
}
// the merge sorts world x width entries per query
int check_shard_width(mi355dr_index* idx, const std::string& what, int width) {
    if ((int64_t)idx->comm_world * width > kSortMax)
        return fail(idx, MI355DR_E_UNSUPPORTED, what + ": world*width exceeds 4096 (width " + std::to_string(width) + ")");
    return MI355DR_OK;
}

// one all-gather of a call: the payload final and visible first (a host transport reads it with copies of its own, ordered
// against the non-blocking stream by nothing), a transport error returned after the stream is drained
int shard_gather(mi355dr_index* idx, hipStream_t s, const void* send, void* recv, size_t bytes_per_rank) {
    HIPCHECK(idx, hipStreamSynchronize(s));
    const int rc = comm_all_gather(idx, send, recv, bytes_per_rank, s);
    if (rc != MI355DR_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    idx->s_shard_gather_bytes += (int64_t)idx->comm_world * (int64_t)bytes_per_rank;
    return MI355DR_OK;
}

int shard_fill_lists(mi355dr_index* idx, hipStream_t s, double* dist, int64_t* rows, int64_t n_entries, int64_t* count, int nb) {
    const int64_t n = std::max<int64_t>(n_entries, nb);
    hipLaunchKernelGGL(k_shard_fill_lists, dim3((unsigned)((n + kShardThreads - 1) / kShardThreads)), dim3(kShardThreads), 0, s,
                       dist, rows, n_entries, count, nb);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// the send / receive buffers for a payload of `words` int64 per rank (before the block's first collective)
int shard_reserve_words(mi355dr_index* idx, size_t words) {
    HIPCHECK(idx, idx->shd.send.grow(words * sizeof(int64_t)));
    HIPCHECK(idx, idx->shd.recv.grow(words * sizeof(int64_t) * (size_t)idx->comm_world));
    return MI355DR_OK;
}

// the sharded search of one block of nb device queries at width w: this shard's list into the packed [2, nb, w] block (plane 0
// the float8 distances, plane 1 global rows), one all-gather, the world*w -> w merge into od / orow [nb, w]
int shard_topk_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int nb, int w, double* od, int64_t* orow) {
    const size_t plane = (size_t)nb * w, words = 2 * plane;
    CHECK(shard_reserve_words(idx, words));
    double* ld = (double*)idx->shd.send.p;
    int64_t* lr = idx->shd.send.p + plane;
    if (idx->n > 0) CHECK(search_block(idx, s, q_dev, nb, w, ld, lr));
    else CHECK(shard_fill_lists(idx, s, ld, lr, (int64_t)plane, nullptr, 0));
    CHECK(shard_gather(idx, s, idx->shd.send.p, idx->shd.recv.p, words * sizeof(int64_t)));
    return launch_merge(idx, (const double*)idx->shd.recv.p, idx->shd.recv.p + plane, (int64_t)words, idx->comm_world, nb, w, od,
                        orow, s);
}

// the sharded range pass of one block: this shard's first m in-range rows and its count into [2, nb, m] + [nb], one
// all-gather (rank stride 2 nb m + nb), the merge of the lists and the sum of the counts
int shard_range_block(mi355dr_index* idx, hipStream_t s, const float* q_dev, int nb, const double* radius, int m, double* od,
                      int64_t* orow, int64_t* ocount) {
    const size_t plane = (size_t)nb * m, words = 2 * plane + nb;
    CHECK(shard_reserve_words(idx, words));
    double* ld = (double*)idx->shd.send.p;
    int64_t* lr = idx->shd.send.p + plane;
    int64_t* lc = idx->shd.send.p + 2 * plane;
    if (idx->n > 0) CHECK(range_block(idx, s, q_dev, nb, radius, m, ld, lr, lc));  // (complete on return)
    else CHECK(shard_fill_lists(idx, s, ld, lr, (int64_t)plane, lc, nb));
    CHECK(shard_gather(idx, s, idx->shd.send.p, idx->shd.recv.p, words * sizeof(int64_t)));
    CHECK(launch_merge(idx, (const double*)idx->shd.recv.p, idx->shd.recv.p + plane, (int64_t)words, idx->comm_world, nb, m, od,
                       orow, s));
    hipLaunchKernelGGL(k_shard_count_fold, dim3((nb + kShardThreads - 1) / kShardThreads), dim3(kShardThreads), 0, s,
                       (const int64_t*)idx->shd.recv.p, (int64_t)words, (int64_t)(2 * plane), idx->comm_world, nb, ocount);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// queries per sub-block of the MMR selection: the gathered stage of the sub-block stays within option "shard_stage_bytes"
int shard_mmr_sub(const mi355dr_index* idx, int nb, int stride) {
    const int64_t per_q = (int64_t)idx->comm_world * stride * (idx->dim + 2) * (int64_t)sizeof(float);
    int64_t qs = std::max<int64_t>(1, std::min<int64_t>(nb, idx->shard_stage_bytes / per_q));
    while (qs > 1 && (int64_t)idx->comm_world * shard_stage_floats(qs * stride, idx->dim) * (int64_t)sizeof(float) > idx->shard_stage_bytes) --qs;
    return (int)qs;
}

// the selection over nb merged lists [nb, stride] in idx->mmr.cand_*: per sub-block the owners stage their candidates'
// vectors and norms, one all-gather, k_shard_mmr_select; asynchronous on the stream behind its last collective
int shard_mmr_block(mi355dr_index* idx, hipStream_t s, int nb, int stride, int k, double lambda, double* out_dist_dev,
                    int64_t* out_rows_dev) {
    const int world = idx->comm_world, qs = shard_mmr_sub(idx, nb, stride);
    const size_t cap_floats = (size_t)shard_stage_floats((int64_t)qs * stride, idx->dim);
    HIPCHECK(idx, idx->shd.stage.grow(cap_floats * sizeof(float)));
    HIPCHECK(idx, idx->shd.stage_all.grow(cap_floats * sizeof(float) * (size_t)world));
    for (int q0 = 0; q0 < nb; q0 += qs) {
        const int nq = std::min(qs, nb - q0);
        const int64_t cnt = (int64_t)nq * stride, rank_floats = shard_stage_floats(cnt, idx->dim);
        const int64_t* crow = idx->mmr.cand_rows.p + (int64_t)q0 * stride;
        hipLaunchKernelGGL(k_shard_mmr_stage, dim3((unsigned)cnt), dim3(kWave), 0, s, crow, cnt, (const float*)idx->rows.p,
                           (const float*)idx->nrm2.p, idx->n, idx->row_offset, idx->dim, idx->shd.stage.p);
        HIPCHECK(idx, hipGetLastError());
        CHECK(shard_gather(idx, s, idx->shd.stage.p, idx->shd.stage_all.p, (size_t)rank_floats * sizeof(float)));
        hipLaunchKernelGGL(k_shard_mmr_select, dim3(nq), dim3(kMmrThreads), mmr_lds_bytes(idx->dim, stride), s, crow,
                           (const double*)idx->mmr.cand_dist.p + (int64_t)q0 * stride, stride, (const float*)idx->shd.stage_all.p,
                           rank_floats, world, cnt, idx->dim, idx->metric, k, lambda, out_dist_dev + (int64_t)q0 * k,
                           out_rows_dev + (int64_t)q0 * k, idx->mmr.pairs_dev.p);
        HIPCHECK(idx, hipGetLastError());
    }
    return MI355DR_OK;
}

// the call's last step of both MMR forms (the stream is idle): the selection's pair counter and the queries into the stats
int shard_mmr_finish(mi355dr_index* idx, int B) {
    unsigned long long pairs = 0;
    HIPCHECK(idx, hipMemcpy(&pairs, idx->mmr.pairs_dev.p, sizeof(pairs), hipMemcpyDeviceToHost));
    idx->s_shard_mmr_searches++;
    idx->s_mmr_queries += B;
    idx->s_mmr_pairs += (int64_t)pairs;
    return MI355DR_OK;
}

// both by-row families over the shards (radius == nullptr: the top-k form), device outputs
int search_rows_sharded_impl(mi355dr_index* idx, const char* what, const int64_t* row_ids, int B, const double* radius, bool range,
                             int kout, int flags, double* out_dist, int64_t* out_rows, int64_t* out_count, void* stream) {
    const bool include_self = (flags & MI355DR_ROWS_INCLUDE_SELF) != 0;
    const int stride = kout + (include_self ? 0 : 1);  // the inner pass's list: room for the row itself
    Call c;
    CHECK(begin_call(idx, what, stream, kCallNoView | kCallDrain, c, [&]() -> int {
        const std::string w(what);
        CHECK(check_comm(idx));
        if (B < 0) return fail(idx, MI355DR_E_INVALID, w + ": B must be >= 0");
        if (kout < 1) return fail(idx, MI355DR_E_INVALID, w + (range ? ": max_results must be >= 1" : ": k must be > 0"));
        if (flags & ~MI355DR_ROWS_INCLUDE_SELF) return fail(idx, MI355DR_E_INVALID, w + ": unknown flag bits");
        if (B > 0 && (!row_ids || !out_dist || !out_rows || (range && (!radius || !out_count))))
            return fail(idx, MI355DR_E_INVALID, w + ": null buffer");
        if (range) CHECK(check_radii(idx, w, radius, B));
        if (stride > kKMax)
            return fail(idx, MI355DR_E_UNSUPPORTED, w + (range ? ": max_results" : ": k") + (include_self ? "" : " + 1 (the row itself)") + " exceeds 1024");
        return check_shard_width(idx, w, stride);
    }));
    if (B == 0) return MI355DR_OK;
    hipStream_t s = c.s;
    const int d = idx->dim, world = idx->comm_world;
    HIPCHECK(idx, idx->rowq.reserve(std::min(B, kQBlockMax), stride, d, /*range=*/true));
    HIPCHECK(idx, grow_each(1, idx->shd.local_skipped));
    HIPCHECK(idx, hipMemsetAsync(idx->rowq.skipped_dev.p, 0, sizeof(unsigned long long), s));
    std::vector<double> rad;
    std::vector<int> valid;
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        // this rank's payload: the owned vectors (zeros elsewhere), valid, the row-with-itself distances (range form; else zeros)
        const int64_t qw = shard_rows_qwords(nb, d), vw = shard_rows_vwords(nb), words = shard_rows_words(nb, d);
        const size_t lists = (size_t)2 * nb * stride + (range ? nb : 0);
        CHECK(shard_reserve_words(idx, std::max((size_t)words, lists)));  // (the inner pass's payload too: nothing grows between the collectives)
        float* pay_q = (float*)idx->shd.send.p;
        int* pay_valid = (int*)(idx->shd.send.p + qw);
        double* pay_self = (double*)(idx->shd.send.p + qw + vw);
        HIPCHECK(idx, hipMemsetAsync(idx->shd.send.p, 0, (size_t)words * sizeof(int64_t), s));  // (the pads and an unused self_dist travel as zeros)
        HIPCHECK(idx, hipMemcpyAsync(idx->rowq.ids.p, row_ids + b0, (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_rows_gather, dim3(nb), dim3(kRowsThreads), 0, s, (const int64_t*)idx->rowq.ids.p, idx->row_offset,
                           idx->n, (const float*)idx->rows.p, (const float*)idx->nrm2.p, d, pay_q, pay_valid, idx->rowq.pair_q.p,
                           idx->rowq.pair_row.p, idx->shd.local_skipped.p);
        HIPCHECK(idx, hipGetLastError());
        if (range && idx->n > 0) {
            // every slot's distance to its own row, on its owner: the bits a search returns for the pair (the others score row 0
            // against zeros, and the fold never reads that)
            HIPCHECK(idx, hipMemcpyAsync(idx->qdev, pay_q, (size_t)nb * d * sizeof(float), hipMemcpyDeviceToDevice, s));
            CHECK(launch_prep(idx, s, nb, (int)round_up(nb, screen_tile(nb)), idx->metric, idle_i8(idx)));
            CHECK(launch_rescore(idx, s, idx->rowq.pair_q.p, idx->rowq.pair_row.p, nb, idx->rowq.self_dot.p, pay_self));
        }
        CHECK(shard_gather(idx, s, idx->shd.send.p, idx->shd.recv.p, (size_t)words * sizeof(int64_t)));
        hipLaunchKernelGGL(k_shard_rows_fold, dim3(nb), dim3(kShardThreads), 0, s, (const int64_t*)idx->shd.recv.p, words, world, nb,
                           d, idx->rowq.q.p, idx->rowq.valid.p, idx->rowq.self_dist.p, idx->rowq.skipped_dev.p);
        HIPCHECK(idx, hipGetLastError());
        if (!range) {
            CHECK(shard_topk_block(idx, s, idx->rowq.q.p, nb, stride, idx->rowq.cand_dist.p, idx->rowq.cand_rows.p));
        } else {
            // a slot nobody owns asks for nothing (its output is blanked below): no row is within -inf
            valid.resize(nb);
            HIPCHECK(idx, hipMemcpyAsync(valid.data(), idx->rowq.valid.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHECK(idx, hipStreamSynchronize(s));
            rad.assign(radius + b0, radius + b0 + nb);
            for (int b = 0; b < nb; ++b)
                if (!valid[b]) rad[b] = -INFINITY;
            HIPCHECK(idx, hipMemcpyAsync(idx->rowq.radius.p, rad.data(), (size_t)nb * sizeof(double), hipMemcpyHostToDevice, s));
            CHECK(shard_range_block(idx, s, idx->rowq.q.p, nb, rad.data(), stride, idx->rowq.cand_dist.p, idx->rowq.cand_rows.p,
                                    idx->rowq.cand_count.p));
        }
        hipLaunchKernelGGL(k_rows_drop, dim3(nb), dim3(kRowsThreads), 0, s, (const double*)idx->rowq.cand_dist.p,
                           (const int64_t*)idx->rowq.cand_rows.p, stride, (const int64_t*)idx->rowq.ids.p,
                           (const int*)idx->rowq.valid.p, kout, include_self ? 1 : 0,
                           range ? (const int64_t*)idx->rowq.cand_count.p : nullptr, (const double*)idx->rowq.self_dist.p,
                           (const double*)idx->rowq.radius.p, out_dist + (int64_t)b0 * kout, out_rows + (int64_t)b0 * kout,
                           range ? out_count + b0 : nullptr);
        HIPCHECK(idx, hipGetLastError());
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the next block reuses the id, query, list and payload buffers)
    }
    unsigned long long skipped = 0;
    HIPCHECK(idx, hipMemcpy(&skipped, idx->rowq.skipped_dev.p, sizeof(skipped), hipMemcpyDeviceToHost));
    idx->s_shard_rows_searches++;
    idx->s_rows_queries += B;
    idx->s_rows_skipped += (int64_t)skipped;
    return MI355DR_OK;
}
}  // namespace

int mi355dr_search_range_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, const double* radius, int max_results,
                                        double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_count_dev, void* stream) {
    const int m = max_results;
    Call c;
    CHECK(begin_call(idx, "search_range_sharded_device", stream, kCallNoView | kCallDrain, c, [&]() -> int {
        CHECK(check_comm(idx));
        if (B <= 0 || m < 1) return fail(idx, MI355DR_E_INVALID, "search_range_sharded_device: B and max_results must be >= 1");
        if (m > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "search_range_sharded_device: max_results exceeds 1024");
        if (!queries_dev || !radius || !out_dist_dev || !out_rows_dev || !out_count_dev)
            return fail(idx, MI355DR_E_INVALID, "search_range_sharded_device: null buffer");
        CHECK(check_radii(idx, "search_range_sharded_device", radius, B));
        return check_shard_width(idx, "search_range_sharded_device", m);
    }));
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        CHECK(shard_range_block(idx, c.s, queries_dev + (int64_t)b0 * idx->dim, nb, radius + b0, m, out_dist_dev + (int64_t)b0 * m,
                                out_rows_dev + (int64_t)b0 * m, out_count_dev + b0));
        HIPCHECK(idx, hipStreamSynchronize(c.s));  // (the next block reuses the payload buffers)
    }
    idx->s_shard_range_searches++;
    idx->s_range_queries += B;
    return MI355DR_OK;
}

int mi355dr_search_rows_sharded_device(mi355dr_index* idx, const int64_t* row_ids, int B, int k, int flags, double* out_dist_dev,
                                       int64_t* out_rows_dev, void* stream) {
    return search_rows_sharded_impl(idx, "search_rows_sharded_device", row_ids, B, nullptr, false, k, flags, out_dist_dev,
                                    out_rows_dev, nullptr, stream);
}

int mi355dr_search_range_rows_sharded_device(mi355dr_index* idx, const int64_t* row_ids, int B, const double* radius,
                                             int max_results, int flags, double* out_dist_dev, int64_t* out_rows_dev,
                                             int64_t* out_count_dev, void* stream) {
    return search_rows_sharded_impl(idx, "search_range_rows_sharded_device", row_ids, B, radius, true, max_results, flags,
                                    out_dist_dev, out_rows_dev, out_count_dev, stream);
}

int mi355dr_search_mmr_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int fetch_k, double lambda,
                                      double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    Call c;
    CHECK(begin_call(idx, "search_mmr_sharded_device", stream, kCallNoView | kCallDrain, c, [&]() -> int {
        CHECK(check_comm(idx));
        CHECK(check_search_args(idx, queries_dev, B, k, out_dist_dev, out_rows_dev));
        CHECK(check_mmr_lambda(idx, "search_mmr_sharded_device", lambda));
        if (fetch_k < k) return fail(idx, MI355DR_E_INVALID, "search_mmr_sharded_device: fetch_k must be >= k");
        if (fetch_k > kMmrMax) return fail(idx, MI355DR_E_UNSUPPORTED, "search_mmr_sharded_device: fetch_k exceeds 1024");
        return check_shard_width(idx, "search_mmr_sharded_device", fetch_k);
    }));
    if (B == 0) return MI355DR_OK;
    HIPCHECK(idx, idx->mmr.reserve(std::min(B, kQBlockMax), fetch_k));
    HIPCHECK(idx, hipMemsetAsync(idx->mmr.pairs_dev.p, 0, sizeof(unsigned long long), c.s));
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        // the sharded search of the block at fetch_k, then the selection over the owners' staged vectors
        CHECK(shard_topk_block(idx, c.s, queries_dev + (int64_t)b0 * idx->dim, nb, fetch_k, idx->mmr.cand_dist.p, idx->mmr.cand_rows.p));
        CHECK(shard_mmr_block(idx, c.s, nb, fetch_k, k, lambda, out_dist_dev + (int64_t)b0 * k, out_rows_dev + (int64_t)b0 * k));
        HIPCHECK(idx, hipStreamSynchronize(c.s));  // (the next block reuses the lists and the stage)
    }
    return shard_mmr_finish(idx, B);
}

// the source-capped search over the shards (section 4.8m): every rank sees the same merged lists, so it takes the same
// decisions and enters the same collectives, round by round
int mi355dr_search_collapsed_sharded_device(mi355dr_index* idx, const float* queries_dev, int B, int k, int cap,
                                            const int64_t* keys_dev, int64_t keys_len, int fetch_k, int max_fetch,
                                            double* out_dist_dev, int64_t* out_rows_dev, int64_t* out_keys_dev,
                                            int32_t* out_count_dev, int32_t* out_state_dev, void* stream) {
    const char* what = "search_collapsed_sharded_device";
    const CollapseSearch a{what, queries_dev, B, k, cap, keys_dev, keys_len, fetch_k, max_fetch, out_dist_dev, out_rows_dev,
                           out_keys_dev, out_count_dev, out_state_dev, stream, /*host=*/false};
    return search_collapsed_impl(
        idx, a, kCallNoView | kCallDrain,
        [&]() -> int {
            CHECK(check_comm(idx));
            return check_shard_width(idx, what, max_fetch);
        },
        // the packed [2, n, f] block of the widest round there can be: a later round (1 x 512 after 5 x 16) never grows it
        [&](int nb_max) { return shard_reserve_words(idx, 2 * (size_t)nb_max * (size_t)max_fetch); },
        [&](hipStream_t s, const float* q, int n, int w, double* od, int64_t* orow) {
            return shard_topk_block(idx, s, q, n, w, od, orow);
        });
}

int mi355dr_mmr_select_sharded(mi355dr_index* idx, const float* queries, int B, int k, const int64_t* cand_rows, int m, double lambda,
                               double* out_dist, int64_t* out_rows) {
    Call c;
    CHECK(begin_call(idx, "mmr_select_sharded", nullptr, kCallNoView | kCallDrain, c, [&]() -> int {
        CHECK(check_comm(idx));
        CHECK(check_search_args(idx, queries, B, k, out_dist, out_rows));
        CHECK(check_mmr_lambda(idx, "mmr_select_sharded", lambda));
        if (m < 0 || (B > 0 && m > 0 && !cand_rows)) return fail(idx, MI355DR_E_INVALID, "mmr_select_sharded: m must be >= 0 and cand_rows not null");
        if (m > kMmrMax) return fail(idx, MI355DR_E_UNSUPPORTED, "mmr_select_sharded: m exceeds 1024");
        return MI355DR_OK;
    }));
    if (B == 0) return MI355DR_OK;
    for (int64_t i = 0; i < (int64_t)B * k; ++i) {
        out_dist[i] = NAN;
        out_rows[i] = -1;
    }
    hipStream_t s = c.s;
    const int world = idx->comm_world;
    HIPCHECK(idx, idx->mmr.reserve(std::min(B, kQBlockMax), std::max(m, 1)));
    HIPCHECK(idx, hipMemsetAsync(idx->mmr.pairs_dev.p, 0, sizeof(unsigned long long), s));
    const CallIO<> io{/*host=*/true, s, nullptr, {out_dist, out_rows, nullptr}, k};
    std::vector<int32_t> pq;
    std::vector<int64_t> pr, first, ordered_rows, mine, all;  // first[b]: query b's first owned pair
    std::vector<double> got, ordered_dist;
    std::vector<MmrCand> list;
    PairBufs bufs;
    for (int b0 = 0; b0 < B && m > 0; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        const size_t plane = (size_t)nb * m;
        try {  // every query's list: the rows THIS shard holds, each once
            pr.clear();
            first.assign(1, 0);
            for (int b = 0; b < nb; ++b) {
                mmr_unique_rows(cand_rows + (int64_t)(b0 + b) * m, m, idx->row_offset, idx->n, pr);
                first.push_back((int64_t)pr.size());
            }
            pq.resize(pr.size());
            for (int b = 0; b < nb; ++b) std::fill(pq.begin() + first[b], pq.begin() + first[b + 1], b);
            got.resize(pr.size());
            mine.assign(2 * plane, -1);  // [2, nb, m]: global rows (-1: not mine / padding -- the flag), distance bits
            all.resize(2 * plane * world);
            ordered_dist.assign(plane, (double)NAN);
            ordered_rows.assign(plane, -1);
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "mmr_select_sharded: out of host memory for the candidate lists");
        }
        CHECK(shard_reserve_words(idx, 2 * plane));
        const int64_t n_pairs = (int64_t)pr.size();
        if (n_pairs > 0)
            CHECK(rescore_host_pairs(idx, bufs, queries + (int64_t)b0 * idx->dim, nb, pq.data(), pr.data(), n_pairs, nullptr, got.data()));
        for (int b = 0; b < nb; ++b)
            for (int64_t i = first[b]; i < first[b + 1]; ++i) {
                const size_t at = (size_t)b * m + (size_t)(i - first[b]);
                mine[at] = pr[i] + idx->row_offset;
                memcpy(&mine[plane + at], &got[i], sizeof(double));  // (a removed row, an undefined distance: the kernel's NaN, and still mine)
            }
        HIPCHECK(idx, hipMemcpyAsync(idx->shd.send.p, mine.data(), 2 * plane * sizeof(int64_t), hipMemcpyHostToDevice, s));
        CHECK(shard_gather(idx, s, idx->shd.send.p, idx->shd.recv.p, 2 * plane * sizeof(int64_t)));
        HIPCHECK(idx, hipMemcpyAsync(all.data(), idx->shd.recv.p, 2 * plane * world * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIPCHECK(idx, hipStreamSynchronize(s));
        // every rank builds the same ordered lists: the union of the ranks' entries (shards are disjoint) in the total order
        try {
            for (int b = 0; b < nb; ++b) {
                list.clear();
                for (int r = 0; r < world; ++r) {
                    const int64_t* rr = all.data() + (size_t)r * 2 * plane + (size_t)b * m;
                    for (int j = 0; j < m && (int)list.size() < m; ++j) {
                        if (rr[j] < 0) continue;
                        double dist;
                        memcpy(&dist, rr + plane + j, sizeof(double));
                        list.push_back(MmrCand{dist, rr[j]});  // (global rows: the same order)
                    }
                }
                mmr_order(list.data(), (int64_t)list.size());
                for (size_t j = 0; j < list.size(); ++j) {
                    ordered_dist[(size_t)b * m + j] = list[j].dist;
                    ordered_rows[(size_t)b * m + j] = list[j].row;
                }
            }
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "mmr_select_sharded: out of host memory for the candidate lists");
        }
        HIPCHECK(idx, hipMemcpyAsync(idx->mmr.cand_dist.p, ordered_dist.data(), plane * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(idx->mmr.cand_rows.p, ordered_rows.data(), plane * sizeof(int64_t), hipMemcpyHostToDevice, s));
        const BlockOut<int64_t> o = block_outputs(idx, io, b0);
        CHECK(shard_mmr_block(idx, s, nb, m, k, lambda, o.dist, o.rows));
        CHECK(block_return(idx, io, b0, nb, o));
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the ordered lists are pageable and are rewritten for the next block)
    }
    HIPCHECK(idx, hipStreamSynchronize(s));
    return shard_mmr_finish(idx, B);
}

int mi355dr_merge_topk_device(mi355dr_index* idx, const double* dist_all_dev, const int64_t* rows_all_dev, int world,
                              int B, int k, double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    return launch_merge(idx, dist_all_dev, rows_all_dev, (int64_t)B * k, world, B, k, out_dist_dev, out_rows_dev, stream);
}

int mi355dr_pack_topk_device(mi355dr_index* idx, const double* dist_dev, const int64_t* rows_dev, int B, int k,
                             int64_t* packed_dev, void* stream) {
    if (!idx || !dist_dev || !rows_dev || !packed_dev) return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B < 0 || k <= 0) return fail(idx, MI355DR_E_INVALID, "bad shape");
    HIPCHECK(idx, hipSetDevice(idx->device));
    hipStream_t s = stream ? (hipStream_t)stream : idx->stream;
    const size_t bytes = (size_t)B * k * 8;
    if (bytes) {
        HIPCHECK(idx, hipMemcpyAsync(packed_dev, dist_dev, bytes, hipMemcpyDeviceToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(packed_dev + (size_t)B * k, rows_dev, bytes, hipMemcpyDeviceToDevice, s));
    }
    return MI355DR_OK;
}

int mi355dr_merge_topk_packed_device(mi355dr_index* idx, const int64_t* packed_all_dev, int world, int B, int k,
                                     double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    return merge_topk_packed(idx, packed_all_dev, world, B, k, out_dist_dev, out_rows_dev, (hipStream_t)stream);
}

// ---- options and stats: one table row each --------------------------------------------------------------------------------
namespace {
using Index = mi355dr_index;

// where an option's value goes: an int, an int64, a switch (an int that holds value != 0) or a double that holds value / 100
struct Field {
    int Index::*i = nullptr;
    int64_t Index::*l = nullptr;
    double Index::*x100 = nullptr;
    bool is_switch = false;
    constexpr Field(int Index::*p, bool is_switch = false) : i(p), is_switch(is_switch) {}
    constexpr Field(int64_t Index::*p) : l(p) {}
    constexpr Field(double Index::*p) : x100(p) {}
    void set(Index* idx, int64_t v) const {
        if (i) idx->*i = is_switch ? v != 0 : (int)v;
        else if (l) idx->*l = v;
        else idx->*x100 = (double)v / 100.0;
    }
};
constexpr bool kSwitch = true;

struct Option {
    const char* key;
    Field field;
    int64_t lo = INT64_MIN, hi = INT64_MAX;  // accepted: lo <= value <= hi ...
    void (*then)(Index*) = nullptr;          // what else a successful set does
    int64_t gap_lo = 0, gap_hi = 0;          // ... but not gap_lo < value < gap_hi
};
const Option kOptions[] = {
    {"path", &Index::path, 0, 2},
    {"screen_dtype", &Index::screen_dtype, 0, 2, [](Index* x) {  // (setting the option again re-arms AUTO)
         x->i8_demoted_k = INT_MAX;
         x->i8_backoff = x->i8_probation = 0;
     }},
    {"i8_min_budget_x100", &Index::i8_min_budget, 1, 1000},
    {"maxsim_screen", {&Index::maxsim_screen, kSwitch}},
    {"maxsim_coop", &Index::maxsim_coop, -1, 1},  // -1: by document length
    {"maxsim_persistent", {&Index::maxsim_persistent, kSwitch}},
    {"maxsim_wg", &Index::maxsim_wg, -1, 2},  // -1: by document length
    {"maxsim_tighten", {&Index::maxsim_tighten, kSwitch}},
    {"maxsim_aligned", {&Index::maxsim_aligned, kSwitch}},
    {"maxsim_wg_min", &Index::maxsim_wg_min, 8, 9},
    {"maxsim_wg_pipe", {&Index::maxsim_wg_pipe, kSwitch}},
    {"maxsim_pack8", &Index::maxsim_pack8, -1, 1},  // -1: when it pays
    {"maxsim_wg_bps", &Index::maxsim_wg_bps, 2, 4, nullptr, 2, 4},  // 2 or 4
    {"maxsim_pass_groups", &Index::maxsim_pass_groups, 1, 4},
    {"maxsim_subset_screen", &Index::maxsim_subset_screen, -1, 1},  // -1: from maxsim_subset_screen_min listed documents on
    {"maxsim_subset_screen_min", &Index::maxsim_subset_screen_min, 0},
    {"row_offset", &Index::row_offset},
    {"profile", {&Index::profile, kSwitch}},
    // (an explicit first chunk means the emit-all ladder: no starter)
    {"chunk0_rows", &Index::chunk0_rows, 1, INT64_MAX, [](Index* x) { x->chunk0_set = 1; }},
    {"starter", {&Index::starter, kSwitch}},
    {"prune_companion", {&Index::prune_companion, kSwitch}},
    {"speculate", {&Index::speculate, kSwitch}, INT64_MIN, INT64_MAX, [](Index* x) { x->spec_backoff = x->spec_probation = 0; }},  // (re-arms)
    {"spec_min_rows", &Index::spec_min_rows, 0},
    {"spec_shift_milli", &Index::spec_shift_milli, -20000, 20000},  // lab: makes the model threshold wrong by this many thousandths of a standard deviation
    {"scan_dma", {&Index::scan_dma, kSwitch}},
    {"defer_round_b", {&Index::defer_round_b, kSwitch}},
    {"chunk_growth", &Index::chunk_growth, 1, INT64_MAX, [](Index* x) { x->chunk_growth_set = 1; }},
    {"screen_stream", {&Index::screen_stream, kSwitch}},
    {"screen_rq", {&Index::screen_rq, kSwitch}},
    {"debug_park_thresholds", &Index::debug_park},
    {"screen_rq_split_tests", {&Index::screen_rq_split_tests, kSwitch}},
    {"screen_drift", &Index::screen_drift, 0, 1024},  // tiles
    {"small_chunk_rows", &Index::small_chunk_rows, 0},
    {"round_a", &Index::round_a, 0, 64},
    {"prefilter16", {&Index::prefilter16, kSwitch}},
    {"cand_cap", &Index::cap, 16, kCandCap, [](Index* x) { x->cap_set = 1; }},
    {"prune_wide", {&Index::prune_wide, kSwitch}},
    {"screen_flush_sync", {&Index::screen_flush_sync, kSwitch}},
    {"screen_flush_lanes", &Index::screen_flush_lanes, 1, 64},
    {"screen_flush_alone", &Index::screen_flush_alone, 8, 60},
    {"wide_inflation_x10", &Index::wide_inflation_x10, 20, 400},
    {"chunk_taper_x100", &Index::chunk_taper_x100, 0, 300, nullptr, 0, 100},  // 0 (auto) or 100 ... 300
    {"starter_rows_wide", &Index::starter_rows_wide, 4096, 262144},
    {"compact_slice_rows", &Index::compact_slice_rows, 32, (int64_t)1 << 22},  // destination rows per staged slice of mi355dr_compact
    {"view_slice_rows", &Index::view_slice_rows, 32, (int64_t)1 << 22},  // rows per staged slice of mi355dr_view_create on this index
    {"range_chunk_rows", &Index::range_chunk_rows, 256, (int64_t)1 << 31},  // rows per screen launch / exact span of mi355dr_search_range (rounded up to 256)
    {"range_slots", &Index::range_slots, 16, kSortMax},  // slots of a query's range result buffer (never below max_results)
    {"sparse_tile_docs", &Index::sparse_tile_docs, 256, 8192},  // documents per LDS tile of k_sparse_score (a power of two: checked below)
    {"sparse_cand_cap", &Index::sparse_cand_cap, 16, 2048},     // slots of a query's sparse candidate list
    {"sparse_overlay_max_pct", &Index::sparse_overlay_max_pct, 0, 100},  // overlay build while moved postings <= this % of the base's (0: never)
    {"sparse_subset_pairs_max", &Index::sparse_subset_pairs_max, 0, 2048},  // longest listed subset looked up pair by pair (<= sparse_cand_cap: checked below)
    {"shard_stage_bytes", &Index::shard_stage_bytes, 1},  // most bytes of the sharded MMR forms' gathered stage (never below one query's)
};

struct Stat {
    const char* key;
    int64_t Index::*counter;                   // a host counter, which mi355dr_reset_stats zeroes if `reset` ...
    bool reset;
    int64_t (*value)(const Index*) = nullptr;  // ... or a value worked out when it is asked for
};
const Stat kStats[] = {
    {"screen_launches", &Index::s_screen_launches, true},
    {"screen_ns", &Index::s_screen_ns, true},
    {"screen_rows", &Index::s_screen_rows, true},
    {"screen256_launches", &Index::s_big_launches, true},
    {"screen_rq_launches", &Index::s_rq_launches, true},
    {"screen256_ns", &Index::s_big_ns, true},
    {"screen256_rows", &Index::s_big_rows, true},
    {"fallback_queries", &Index::s_fallback_queries, true},
    {"chunks", &Index::s_chunks, true},
    {"passes", &Index::s_passes, true},
    {"starters", &Index::s_starters, true},
    {"retry_queries", &Index::s_retry_queries, true},
    {"spec_passes", &Index::s_spec_passes, true},
    {"spec_miss_queries", &Index::s_spec_miss_queries, true},
    {"spec_overflow_queries", &Index::s_spec_overflow_queries, true},
    {"spec_suspended", nullptr, false, [](const Index* x) -> int64_t { return x->spec_probation > 0 ? 1 : 0; }},
    {"maxsim_screened", &Index::s_ms_screened, true},
    {"maxsim_candidates", &Index::s_ms_candidates, true},
    {"maxsim_fallbacks", &Index::s_ms_fallbacks, true},
    {"maxsim_screen_ns", &Index::s_ms_screen_ns, true},
    {"maxsim_pack_ns", &Index::s_ms_pack_ns, true},
    {"maxsim_screen_launches", &Index::s_ms_screen_launches, true},
    {"maxsim_exact_ns", &Index::s_ms_exact_ns, true},
    {"maxsim_exact_launches", &Index::s_ms_exact_launches, true},
    {"maxsim_screen_cols", &Index::s_ms_screen_cols, true},
    {"maxsim_packed_launches", &Index::s_ms_packed_launches, true},
    {"maxsim_packed_blocks", &Index::s_ms_packed_blocks, false},  // (the packed copy's size and its build history: state, not activity)
    {"maxsim_packed_built", &Index::s_ms_packed_built, false},
    {"maxsim_set_docs", &Index::s_ms_set_docs, true},
    {"maxsim_moved_blocks", &Index::s_ms_moved_blocks, true},
    {"subset_searches", &Index::s_subset_searches, true},
    {"subset_rows_scored", &Index::s_subset_rows_scored, true},
    {"subset_rerun_queries", &Index::s_subset_rerun_queries, true},
    {"maxsim_subset_searches", &Index::s_mss_searches, true},
    {"maxsim_subset_docs", &Index::s_mss_docs, true},
    {"maxsim_subset_screened", &Index::s_mss_screened, true},
    {"maxsim_subset_exact", &Index::s_mss_exact, true},
    {"maxsim_subset_fallbacks", &Index::s_mss_fallbacks, true},
    {"maxsim_align_calls", &Index::s_msa_calls, true},
    {"maxsim_align_pairs", &Index::s_msa_pairs, true},
    {"maxsim_map_calls", &Index::s_msm_calls, true},
    {"maxsim_map_values", &Index::s_msm_values, true},
    {"mmr_searches", &Index::s_mmr_searches, true},
    {"mmr_queries", &Index::s_mmr_queries, true},
    {"mmr_pairs_scored", &Index::s_mmr_pairs, true},
    {"group_searches", &Index::s_group_searches, true},
    {"group_subqueries", &Index::s_group_subqueries, true},
    {"groups_merged", &Index::s_groups_merged, true},
    {"fuse_calls", &Index::s_fuse_calls, true},
    {"fuse_queries", &Index::s_fuse_queries, true},
    {"collapse_calls", &Index::s_collapse_calls, true},
    {"collapse_searches", &Index::s_collapse_searches, true},
    {"collapse_queries", &Index::s_collapse_queries, true},
    {"collapse_researched", &Index::s_collapse_researched, true},
    {"collapse_truncated", &Index::s_collapse_truncated, true},
    {"range_searches", &Index::s_range_searches, true},
    {"range_queries", &Index::s_range_queries, true},
    {"range_in_range", &Index::s_range_in_range, true},
    {"range_candidates", &Index::s_range_candidates, true},
    {"range_rescored", &Index::s_range_rescored, true},
    {"range_redo_chunks", &Index::s_range_redo_chunks, true},
    {"range_fallback_queries", &Index::s_range_fallback_queries, true},
    {"rows_searches", &Index::s_rows_searches, true},
    {"rows_queries", &Index::s_rows_queries, true},
    {"rows_skipped", &Index::s_rows_skipped, true},
    {"examples_searches", &Index::s_examples_searches, true},
    {"examples_queries", &Index::s_examples_queries, true},
    {"examples_skipped", &Index::s_examples_skipped, true},
    {"examples_skipped_slots", &Index::s_examples_skipped_slots, true},
    {"feedback_searches", &Index::s_feedback_searches, true},
    {"sharded_range_searches", &Index::s_shard_range_searches, true},
    {"sharded_rows_searches", &Index::s_shard_rows_searches, true},
    {"sharded_mmr_searches", &Index::s_shard_mmr_searches, true},
    {"shard_gather_bytes", &Index::s_shard_gather_bytes, true},
    {"sharded_sparse_searches", &Index::s_shard_sparse_searches, true},
    {"sharded_sparse_scores", &Index::s_shard_sparse_scores, true},
    {"sparse_searches", &Index::s_sparse_searches, true},
    {"sparse_queries", &Index::s_sparse_queries, true},
    {"sparse_postings_scored", &Index::s_sparse_postings_scored, true},
    {"sparse_overflows", &Index::s_sparse_overflows, true},
    {"sparse_full_builds", &Index::s_sparse_full_builds, true},
    {"sparse_overlay_builds", &Index::s_sparse_overlay_builds, true},
    {"sparse_sets", &Index::s_sparse_sets, true},
    {"sparse_subset_searches", &Index::s_sparse_subset_searches, true},
    {"sparse_subset_scores", &Index::s_sparse_subset_scores, true},
    {"sparse_subset_pairs", &Index::s_sparse_subset_pairs, true},
    {"sparse_subset_tiles", &Index::s_sparse_subset_tiles, true},
    {"sparse_overlay_postings", nullptr, false, [](const Index* x) -> int64_t { return sparse_stat(x, kSparseStatOverlayPostings); }},
    {"sparse_dead_postings", nullptr, false, [](const Index* x) -> int64_t { return sparse_stat(x, kSparseStatDeadPostings); }},
    {"sparse_docs", nullptr, false, [](const Index* x) -> int64_t { return sparse_stat(x, kSparseStatDocs); }},
    {"sparse_total_len", nullptr, false, [](const Index* x) -> int64_t { return sparse_stat(x, kSparseStatTotalLen); }},
    {"sparse_postings", nullptr, false, [](const Index* x) -> int64_t { return sparse_stat(x, kSparseStatPostings); }},
    {"sparse_vocab", nullptr, false, [](const Index* x) -> int64_t { return sparse_stat(x, kSparseStatVocab); }},
    {"compactions", &Index::s_compactions, true},
    {"compact_moved_rows", &Index::s_compact_moved_rows, true},
    {"view", nullptr, false, [](const Index* x) -> int64_t { return x->is_view ? 1 : 0; }},
    {"view_rows", &Index::view_rows, false},  // (what mi355dr_view_create kept: state, not activity; 0 on a parent)
    {"view_docs", &Index::view_docs, false},
    {"i8_demoted", nullptr, false, [](const Index* x) -> int64_t { return x->i8_demoted_k != INT_MAX ? 1 : 0; }},
    {"i8_demoted_k", nullptr, false, [](const Index* x) -> int64_t { return x->i8_demoted_k == INT_MAX ? 0 : x->i8_demoted_k; }},
    {"irregular_rows", nullptr, false, [](const Index* x) -> int64_t { return x->irr_n; }},
    {"loose_rows", nullptr, false, [](const Index* x) -> int64_t { return x->irr8_n; }},
    {"dead_rows", nullptr, false, [](const Index* x) -> int64_t { return x->dead_n; }},
    {"screen_dtype_active", nullptr, false, [](const Index* x) -> int64_t { return idle_i8(x) ? MI355DR_SCREEN_I8 : MI355DR_SCREEN_BF16; }},
    {"hbm_bytes_resident", nullptr, false, [](const Index* x) -> int64_t {
         return x->cap_rows * ((int64_t)x->dim * 4 + (int64_t)x->dpad * 2 + (int64_t)x->dpad8 + 5) +
                x->cap_rows / kI8GroupRows * (int64_t)sizeof(I8Group) + multivec_bytes(x) +
                (int64_t)(x->view_row_map.bytes + x->view_doc_map.bytes) +  // (a view's two id maps; none on a parent)
                sparse_bytes(x) + (int64_t)x->clp.bytes();  // (the source-capped forms' staging and block state, as grown)
     }},
};
}  // namespace

int mi355dr_debug_spec_m(int k) { return spec_m_of(k); }  // (no index, no device: tests/test_spec_model.py holds it to the rule)

int mi355dr_set_option(mi355dr_index* idx, const char* key, int64_t value) {
    if (!idx || !key) return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->seq_done < idx->seq_next) {  // (a fix-up of a block in flight must see the options it was enqueued under)
        HIPCHECK(idx, hipSetDevice(idx->device));
        CHECK(drain_pending(idx));
    }
    if (idx->is_view && strcmp(key, "row_offset") == 0) return view_refuses(idx, "option row_offset");  // (its rows are the parent's ids)
    for (const Option& o : kOptions) {
        if (strcmp(o.key, key) != 0) continue;
        if (value < o.lo || value > o.hi || (value > o.gap_lo && value < o.gap_hi)) {
            std::string range = o.hi == INT64_MAX ? " must be >= " + std::to_string(o.lo)
                                                  : " must be in [" + std::to_string(o.lo) + ", " + std::to_string(o.hi) + "]";
            if (o.gap_lo < o.gap_hi) range += ", not between " + std::to_string(o.gap_lo) + " and " + std::to_string(o.gap_hi);
            return fail(idx, MI355DR_E_INVALID, o.key + range);
        }
        if (strcmp(key, "sparse_tile_docs") == 0 && (value & (value - 1)) != 0)
            return fail(idx, MI355DR_E_INVALID, "sparse_tile_docs must be a power of two");
        if (strcmp(key, "sparse_subset_pairs_max") == 0 && value > idx->sparse_cand_cap)
            return fail(idx, MI355DR_E_INVALID, "sparse_subset_pairs_max must not exceed sparse_cand_cap");
        o.field.set(idx, value);
        if (o.then) o.then(idx);
        return MI355DR_OK;
    }
    return fail(idx, MI355DR_E_INVALID, std::string("unknown option: ") + key);
}

int mi355dr_get_stat(mi355dr_index* idx, const char* key, int64_t* out) {
    if (!idx || !key || !out) return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    const std::string k(key);
    if (k == "candidates" || k == "rescored") {  // the two counters the prunes keep on the device, per query
        unsigned long long v[2] = {0, 0};
        if (idx->stat_dev) {
            std::vector<unsigned long long> per(2 * kQBlockMax);
            HIPCHECK(idx, hipSetDevice(idx->device));
            HIPCHECK(idx, hipMemcpy(per.data(), idx->stat_dev, per.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int i = 0; i < kQBlockMax; ++i) {
                v[0] += per[2 * i];
                v[1] += per[2 * i + 1];
            }
        }
        *out = (int64_t)(k == "candidates" ? v[0] : v[1]);
        return MI355DR_OK;
    }
    for (const Stat& st : kStats) {
        if (k != st.key) continue;
        *out = st.counter ? idx->*st.counter : st.value(idx);
        return MI355DR_OK;
    }
    return fail(idx, MI355DR_E_INVALID, "unknown stat: " + k);
}

int mi355dr_reset_stats(mi355dr_index* idx) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    for (const Stat& st : kStats)
        if (st.reset) idx->*st.counter = 0;
    if (idx->stat_dev) {
        HIPCHECK(idx, hipSetDevice(idx->device));
        HIPCHECK(idx, hipMemset(idx->stat_dev, 0, 2 * kQBlockMax * sizeof(unsigned long long)));
    }
    return MI355DR_OK;
}

int mi355dr_timer_start(mi355dr_index* idx) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipEventRecord(idx->t0, idx->stream));
    return MI355DR_OK;
}
int mi355dr_timer_stop(mi355dr_index* idx, double* elapsed_ms) {
    if (!idx || !elapsed_ms) return fail(idx, MI355DR_E_INVALID, "null argument");
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipEventRecord(idx->t1, idx->stream));
    HIPCHECK(idx, hipEventSynchronize(idx->t1));
    float ms = 0.f;
    HIPCHECK(idx, hipEventElapsedTime(&ms, idx->t0, idx->t1));
    *elapsed_ms = ms;
    return MI355DR_OK;
}
int mi355dr_synchronize(mi355dr_index* idx) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipStreamSynchronize(idx->stream));
    return MI355DR_OK;
}

int mi355dr_dev_alloc(mi355dr_index* idx, size_t bytes, void** out) {
    if (!idx || !out) return fail(idx, MI355DR_E_INVALID, "null argument");
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipMalloc(out, bytes ? bytes : 1));
    return MI355DR_OK;
}
int mi355dr_dev_free(mi355dr_index* idx, void* p) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    HIPCHECK(idx, hipSetDevice(idx->device));
    if (p) HIPCHECK(idx, hipFree(p));
    return MI355DR_OK;
}
int mi355dr_dev_upload(mi355dr_index* idx, void* dst_dev, const void* src_host, size_t bytes) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return MI355DR_OK;
}
int mi355dr_dev_download(mi355dr_index* idx, void* dst_host, const void* src_dev, size_t bytes) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return MI355DR_OK;
}

int mi355dr_debug_screen_dense(mi355dr_index* idx, const float* queries, int B, int64_t row0, int64_t n, float* out_t) {
    if (!idx || !queries || !out_t) return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B <= 0 || B > kQBlockMax || n <= 0 || n > kCandCap || row0 < 0 || row0 % screen_tile(B) != 0 || row0 + n > idx->n)
        return fail(idx, MI355DR_E_INVALID,
                    "debug_screen_dense: need 1<=B<=1024, 1<=n<=2048, row0 a multiple of the tile (128; 256 if B>128)");
    CHECK(upload_and_prep(idx, queries, B, /*metric=*/2));  // test hook: thresholds at -inf for every query
    hipStream_t s = idx->stream;
    const bool i8 = idle_i8(idx);
    CHECK(launch_screen(idx, s, i8, B, row0, row0 + n, kCandCap, /*emit_mode=*/0, /*flush_mask=*/-1));
    std::vector<int> cnt(B);
    std::vector<int32_t> crow((size_t)B * kCandCap);
    std::vector<float> cval((size_t)B * kCandCap);
    HIPCHECK(idx, hipMemcpyAsync(cnt.data(), idx->st.cnt, B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(crow.data(), idx->cand_row, crow.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(cval.data(), idx->cand_val, cval.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    std::vector<uint8_t> flag(n, 0);  // int8 screen: rows outside the shadow carry a stale 0 (k_prune drops them)
    if (i8) HIPCHECK(idx, hipMemcpyAsync(flag.data(), idx->flag8 + row0, n, hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    for (int64_t i = 0; i < (int64_t)B * n; ++i) out_t[i] = NAN;
    for (int b = 0; b < B; ++b) {
        const int c = std::min(cnt[b], kCandCap);
        for (int j = 0; j < c; ++j) {
            const int64_t r = crow[(size_t)b * kCandCap + j] - row0;
            if (r >= 0 && r < n && !flag[r]) out_t[(int64_t)b * n + r] = cval[(size_t)b * kCandCap + j];
        }
    }
    return MI355DR_OK;
}

int mi355dr_debug_screen_hits(mi355dr_index* idx, const float* queries, int B, int64_t row0, int64_t n, const float* thr,
                              int cap, int* out_count, int32_t* out_rows, float* out_vals, int* out_status, int* out_kernel) {
    if (!idx || !queries || !thr || !out_count || !out_rows || !out_vals || !out_status || !out_kernel)
        return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B <= 0 || B > kQBlockMax || n <= 0 || row0 < 0 || row0 % screen_tile(B) != 0 || row0 + n > idx->n || cap < 16 ||
        cap > kCandCapWide)
        return fail(idx, MI355DR_E_INVALID,
                    "debug_screen_hits: need 1<=B<=1024, n>=1, row0 a multiple of the tile (128; 256 if B>128), 16<=cap<=4096");
    for (int b = 0; b < B; ++b)
        if (!(thr[b] < INFINITY))  // (NaN compares false)
            return fail(idx, MI355DR_E_INVALID, "debug_screen_hits: thresholds must be finite or -inf");
    CHECK(upload_and_prep(idx, queries, B, /*metric=*/2));  // (queries behind B, padding of the last tile: thresholds at +inf)
    hipStream_t s = idx->stream;
    HIPCHECK(idx, hipMemcpyAsync(idx->st.thr, thr, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    // k_screen_rq's synchronised flushes: run_screen derives the period from k and the rows seen, neither of which exists
    // here -- two tiles, so that a workgroup of a few visits takes both the common flush and (at flush_alone) a wave's own
    const bool i8 = idle_i8(idx);
    *out_kernel = (int)screen_kernel_for(idx, i8, B, n, /*emit_all=*/false);
    CHECK(launch_screen(idx, s, i8, B, row0, row0 + n, cap, /*emit_mode=*/0, idx->screen_flush_sync ? 1 : -1));
    HIPCHECK(idx, hipMemcpyAsync(out_count, idx->st.cnt, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(out_status, idx->st.status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(out_rows, idx->cand_row, (size_t)B * cap * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(out_vals, idx->cand_val, (size_t)B * cap * sizeof(float), hipMemcpyDeviceToHost, s));
    std::vector<uint8_t> flag;  // int8 screen: rows outside the shadow carry a stale 0 (k_prune drops them)
    if (i8) {
        flag.resize((size_t)n);
        HIPCHECK(idx, hipMemcpyAsync(flag.data(), idx->flag8 + row0, (size_t)n, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(idx, hipStreamSynchronize(s));
    if (!flag.empty())
        for (int b = 0; b < B; ++b) {
            const int c = std::min(std::max(out_count[b], 0), cap);
            for (int j = 0; j < c; ++j) {
                int32_t& r = out_rows[(size_t)b * cap + j];
                if (r >= row0 && r < row0 + n && flag[(size_t)(r - row0)]) r = -1 - r;
            }
        }
    return MI355DR_OK;
}

int mi355dr_debug_screen_bound(mi355dr_index* idx, const float* queries, int B, float* out_E) {
    if (!idx || !queries || !out_E) return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B <= 0 || B > kQBlockMax) return fail(idx, MI355DR_E_INVALID, "need 1<=B<=1024");
    CHECK(upload_and_prep(idx, queries, B, idx->metric));
    hipStream_t s = idx->stream;
    HIPCHECK(idx, hipMemcpyAsync(out_E, idx->st.E, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    return MI355DR_OK;
}

int mi355dr_debug_i8_state(mi355dr_index* idx, const float* queries, int B, float* out_sq, float* out_kq, int64_t g0,
                           int64_t n_groups, float* out_step, float* out_err) {
    if (!idx || !queries || !out_sq || !out_kq || !out_step || !out_err) return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B <= 0 || B > kQBlockMax) return fail(idx, MI355DR_E_INVALID, "need 1<=B<=1024");
    if (g0 < 0 || n_groups < 0 || (g0 + n_groups) * kI8GroupRows > idx->cap_rows)
        return fail(idx, MI355DR_E_INVALID, "group range outside the index");
    if (!idle_i8(idx)) return fail(idx, MI355DR_E_UNSUPPORTED, "the int8 screen is not active");
    CHECK(upload_and_prep(idx, queries, B, idx->metric));
    hipStream_t s = idx->stream;
    HIPCHECK(idx, hipMemcpyAsync(out_sq, idx->st.sc, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(out_kq, idx->st.kq, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
    std::vector<I8Group> gr((size_t)n_groups);
    if (n_groups > 0)
        HIPCHECK(idx, hipMemcpyAsync(gr.data(), idx->grp8 + g0, (size_t)n_groups * sizeof(I8Group), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    for (int64_t i = 0; i < n_groups; ++i) {
        out_step[i] = gr[(size_t)i].step;
        out_err[i] = gr[(size_t)i].err;
    }
    return MI355DR_OK;
}

int mi355dr_debug_spec_model(mi355dr_index* idx, const float* queries, int B, int k, float* out_moments, float* out_thr_rigorous,
                             float* out_thr_used, double* out_zq, int64_t* out_sample_rows, int* out_slabs, int* out_i8) {
    if (!idx || !queries || !out_moments || !out_thr_rigorous || !out_thr_used || !out_zq || !out_sample_rows || !out_slabs ||
        !out_i8)
        return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B <= 0 || B > kQBlockMax || k <= 0 || k > kKMax) return fail(idx, MI355DR_E_INVALID, "need 1<=B<=1024, 1<=k<=1024");
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_pending(idx));
    CHECK(ensure_qstate(idx));
    const Pass ps = decide_pass(idx, k, 0, false, "screen path unavailable (metric or too many irregular rows)");
    if (ps.refused) return fail(idx, MI355DR_E_UNSUPPORTED, ps.refused);
    if (!ps.speculative) return fail(idx, MI355DR_E_UNSUPPORTED, "debug_spec_model: a pass at this k would not speculate");
    idx->last_pass_k = k;  // (as a search at k leaves it: the other hooks then read the screen this pass took)
    hipStream_t s = idx->stream;
    const PassPlan plan = make_plan(idx, ps, B);
    const SpecModel sm = spec_model(idx, ps, plan, out_zq);
    const int Bpad = (int)round_up(B, screen_tile(B));
    // the prunes count candidates and re-scored rows per query on the device (stats "candidates", "rescored"): the hook hands
    // the words back as it found them, also where a launch below fails
    std::vector<unsigned long long> stat_before(2 * (size_t)kQBlockMax);
    const size_t stat_bytes = stat_before.size() * sizeof(unsigned long long);
    HIPCHECK(idx, hipMemcpyAsync(stat_before.data(), idx->stat_dev, stat_bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    // the head of run_screen, twice: the plain starter (what the rigorous threshold is), then the speculative pass's
    const auto heads = [&]() -> int {
        for (int model = 0; model < 2; ++model) {
            HIPCHECK(idx, hipMemcpyAsync(idx->qdev, queries, (size_t)B * idx->dim * sizeof(float), hipMemcpyHostToDevice, s));
            CHECK(launch_prep(idx, s, B, Bpad, idx->metric, ps.i8, starter_count(plan)));
            CHECK(launch_screen(idx, s, ps.i8, B, 0, plan.sample, ps.cap, kEmitSlabMax, -1, model ? sm.slabs : 0));
            CHECK(launch_prune(idx, s, ps, B, nullptr, /*exact=*/0, /*thr_only=*/true, /*one_wave_only=*/true, false,
                               model ? &sm : nullptr));
            if (!model)
                HIPCHECK(idx, hipMemcpyAsync(out_thr_rigorous, idx->st.thr, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        HIPCHECK(idx, hipMemcpyAsync(out_thr_used, idx->st.thr_used, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHECK(idx, hipMemcpyAsync(out_moments, idx->spec_moments, (size_t)B * sm.slabs * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
        return MI355DR_OK;
    };
    const int rc = heads();
    const hipError_t put_back = hipMemcpyAsync(idx->stat_dev, stat_before.data(), stat_bytes, hipMemcpyHostToDevice, s);
    const hipError_t done = hipStreamSynchronize(s);
    CHECK(rc);
    HIPCHECK(idx, put_back);
    HIPCHECK(idx, done);
    *out_sample_rows = plan.sample;
    *out_slabs = sm.slabs;
    *out_i8 = ps.i8 ? 1 : 0;
    return MI355DR_OK;
}

int mi355dr_debug_rescore(mi355dr_index* idx, const float* queries, int B, const int32_t* pair_q,
                          const int64_t* pair_row, int64_t n_pairs, float* out_dot, double* out_dist) {
    if (!idx || !queries || !pair_q || !pair_row || !out_dot || !out_dist)
        return fail(idx, MI355DR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B <= 0 || B > kQBlockMax || n_pairs <= 0) return fail(idx, MI355DR_E_INVALID, "bad shape");
    for (int64_t i = 0; i < n_pairs; ++i)
        if (pair_q[i] < 0 || pair_q[i] >= B || pair_row[i] < 0 || pair_row[i] >= idx->n)
            return fail(idx, MI355DR_E_INVALID, "pair out of range");
    PairBufs bufs;
    return rescore_host_pairs(idx, bufs, queries, B, pair_q, pair_row, n_pairs, out_dot, out_dist);
}

/* ---- multi-vector (MaxSim): implemented in mi355dr_maxsim.hip ---- */

}  // extern "C"
