// mi355dr_maxsim.hip -- multi-vector (late interaction) store and exact MaxSim top-k: the host side.
// Kernels: k_maxsim_exact.h (k_maxsim), k_maxsim_align.h (the terms of its sum: alignment and maps), k_maxsim_select.h (selection),
// k_maxsim_build.h (store images); the bf16 screens live in mi355dr_maxsim_screen.hip.
//
// Replaces VectorChord's `embeddings @# ARRAY[q_1..q_n]` + ORDER BY distance LIMIT k
// (reference autorag_research/orm/repository/base.py:487-535, :537-571):
//     distance(doc) = sum_i min_j ( -<q_i, d_j> )      fp32; score = -distance / n_q on the host
// with every dot product the k-ascending fp32 fmaf chain (oracle.c orc_maxsim_distance), the sum over
// query vectors in query order.  Bit-exact by construction: v_mfma_f32_32x32x2_f32 IS a k-ordered
// fmaf chain per output element (MI355X guide: "bit-for-bit a k-ordered f32 fmaf chain"), max is
// exact, and the final sum is done sequentially in j.
//
// HBM layout: doc token rows are stored padded so that every doc owns whole 32-row blocks; the tail of
// the last block repeats the doc's last token (max over a multiset with repeats is unchanged), and the
// vector dimension is zero-padded to a multiple of 8 (fma(0,0,acc) == acc).  One wave owns one doc:
// each 32-row block x 32 query tokens is one chain of d/2 MFMAs; operands go global -> VGPR as float4
// (A, doc tokens) and LDS -> VGPR (B, query tokens), and two v_permlane32_swap per 4 MFMAs put k in
// ascending order.  fp32 MFMA runs at the vector rate (157 TF peak): at one 32-token query per pass the
// kernel is at the HBM/MFMA balance point (16 flop/B), with more queries per pass it is MFMA-bound.
//
// Search = bf16 MFMA screen over every doc (k_maxsim16, HBM-bound on a bf16 copy of the tokens laid out in MFMA
// fragment order) -> candidates under a rigorous bound -> exact kernel (k_maxsim, doc list) on the candidates ->
// exact top-k.  Same results as running the exact kernel over every doc (option "maxsim_screen" = 0), which stays
// the path for stores / queries with non-finite values and for candidate lists that overflow.
//   bound (a priori): every token pair |t_ij - s_ij| <= eps |q_i||d_j|, eps = 2^-7 + 2^-15 + 3 d 2^-24 (bf16 rounding of both
//   sides + fp32 accumulation + the exact chain's own rounding), so |max_j t_ij - max_j s_ij| <= eps |q_i| Dmax
//   (Dmax = largest token norm in the store) and |T - S| <= E = (eps + 2 n_q 2^-24) Dmax sum_i |q_i| for the
//   per-doc sums.  k docs have T >= x_k (k-th best screen score) hence S >= x_k - E; any doc of the exact top-k
//   (ties included) has S >= that, hence T >= x_k - 2E: the candidate set.
#include <chrono>

#include "maxsim_common.h"
#include "subset_ids.h"

#include "k_maxsim_build.h"
#include "k_maxsim_exact.h"
#include "k_maxsim_align.h"
#include "k_maxsim_select.h"

using namespace mi355;

namespace mi355 {

// Every buffer is a DevBuf (index.h): the store is released by `delete`, and a buffer that failed to grow is still the old one.
struct MultiVecStore {
    int64_t n_docs = 0;
    int64_t n_blocks = 0, cap_blocks = 0;  // 32-row blocks stored / allocated
    int64_t cap_docs = 0;
    int dpad = 0;                  // dim rounded up to 8
    DevBuf<float> tok;             // [cap_blocks*32, dpad]
    // bf16 copy for the screen, MFMA fragment order: [block][kk][lane][8] with lane = (row = lane&31, half = lane>>5)
    // holding dims kk*16 + half*8 + 0..7 of token `row` (original column order)
    int nkk = 0;                   // dim rounded up to 16, / 16
    DevBuf<uint4> tok16;           // [cap_blocks * nkk * 64]
    double tok_norm_max = 0.0;     // largest token norm (double, from the fp32 values)
    double tok16_norm_max = 0.0;   // largest norm of a bf16-rounded token
    double tok_res_max = 0.0;      // largest residual norm |d - bf16(d)| of a token
    bool finite = true;            // every stored value is finite (else: no screen)
    DevBuf<int64_t> blk_off;       // [cap_docs+1] first block of each doc (device)
    std::vector<int64_t> blk_off_host;
    std::vector<int32_t> tok_cnt_host;  // [n_docs] token vectors of each doc (the padded copies do not keep it)
    int64_t n_live = 0;                 // docs that have vectors (a removed doc is a doc without: mi355dr_set_multivec)
    // the granule-packed bf16 copy of k_maxsim_wg8.h: a second shadow, built on first use (ms_pack8_ensure), stale after an add
    // (extended by the next pass that takes it) and after a set (pack_docs = -1: packed whole)
    DevBuf<uint4> tok16p;          // [pack_cap_blocks * nkk * 64]
    DevBuf<int64_t> goff;          // [pack_cap_docs + 1] first 8-token granule of each doc (device)
    int64_t pack_docs = -1;        // n_docs the copy was built (or judged) for; -1: never
    int64_t pack_gran = 0, pack_blocks = 0, pack_cap_blocks = 0, pack_cap_docs = 0;
    bool pack_use = false;         // the copy exists for pack_docs docs and pays (or is forced)
    int pack_mode = 0;             // option maxsim_pack8 at the time of that decision
    // search scratch of fixed size (ms_search_prepare; scratch_ready is set after the last of them is there)
    bool scratch_ready = false;
    DevBuf<float> qtok;            // [kMsImgCols, dpad] fp32 query image of a pass
    DevBuf<uint4> qfrag;           // [kMsPassBlocks * nkk * 64] query fragments of one screen launch (up to four groups of <= 4 queries)
    // candidate lists of a pass, per query (row stride kMsCandCap): section 0 = the WIDE list (screen distance within 2E of the
    // k-th best), 1 = the STARTER (the screen's own top-k), 2 = the FINAL list (within E of the starter's k-th best exact distance)
    DevBuf<int32_t> cand_list;     // [3][kMsPassQueries][kMsCandCap]
    DevBuf<float> cand_dist;       // [kMsPassQueries][kMsCandCap] exact distances of the list being re-scored (starter, then final)
    DevBuf<float> cand_sd;         // [kMsPassQueries][kMsCandCap] screen distances of the wide list's entries
    DevBuf<int> cand_ctl;          // [3][kMsPassQueries][2]: count, overflow flag
    HostBuf<int> cand_ctl_host;    // pinned [2 * kMsPassQueries]: the final list's
    DevBuf<float> two_e_dev;       // [kMsPassQueries]
    DevBuf<float> out_d;           // [kMsPassQueries, kKMax]
    DevBuf<int64_t> out_r;
    HostBuf<char> stage_host;      // pinned: query image | query fragments | 2E (H2D), results (D2H)
    // search scratch that follows the store's size (each grows by its own size)
    DevBuf<float> dist;            // [max queries per launch (4), cap_docs]
    DevBuf<float> dist16;          // [kMsPassQueries, cap_docs] screen distances (rows 4 g ..: the groups screened ahead)
    DevBuf<uint32_t> sel[2];       // fast path: per-segment k best screen keys, [kMsPassQueries, ceil(cap_docs/1024) * 64]
    DevBuf<uint64_t> pk[2];        // segment-wise top-k partials (ms_topk)
    DevBuf<int32_t> pr[2];
    // mi355dr_search_maxsim_subset, the call in progress: the listed documents with vectors (local, ascending, unique) and the
    // membership table T[0 .. n_docs], T[d] = listed documents below d (k_ms_membership)
    DevBuf<int32_t> sub_list;
    DevBuf<int64_t> sub_memb;
};

bool multivec_view(const mi355dr_index* idx, MultiVecView* out) {
    const MultiVecStore* m = idx->mv;
    if (!m || m->n_docs == 0) return false;
    out->tok = m->tok.p;
    out->blk_off = m->blk_off.p;
    out->blk_off_host = m->blk_off_host.data();
    out->tok_cnt_host = m->tok_cnt_host.data();
    out->dpad = m->dpad;
    out->n_docs = m->n_docs;
    return true;
}

// device bytes of the store's images, offset table and granule-packed copy as they are allocated now (the buffers' own sizes: a
// relayout's swap, a regrow and a released packed copy are all reflected)
int64_t multivec_bytes(const mi355dr_index* idx) {
    const MultiVecStore* m = idx->mv;
    return m ? (int64_t)(m->tok.bytes + m->tok16.bytes + m->blk_off.bytes + m->tok16p.bytes + m->goff.bytes) : 0;
}

void multivec_destroy(mi355dr_index* idx) {
    delete idx->mv;
    idx->mv = nullptr;
}

}  // namespace mi355

namespace {

inline float host_bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

inline uint16_t host_bf16_rn(float f) {  // round-to-nearest-even; NaN/Inf keep their class (the screen is off for them)
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// ---- the store: one builder behind both add entry points --------------------------------------------------------------------

// `buf` -> a block of new_bytes that starts with its first keep_bytes: allocate, copy, then swap (a failed copy frees the new block)
template <class T>
int ms_regrow(mi355dr_index* idx, DevBuf<T>& buf, size_t new_bytes, size_t keep_bytes) {
    DevBuf<T> t;
    HIPCHECK(idx, t.grow(new_bytes));
    if (keep_bytes > 0) HIPCHECK(idx, hipMemcpy(t.p, buf.p, keep_bytes, hipMemcpyDeviceToDevice));
    buf.swap(t);
    return MI355DR_OK;
}

// room for want_blocks blocks and want_docs docs; what is stored stays.  A capacity is written after its buffers are there.
int ms_reserve(mi355dr_index* idx, MultiVecStore* m, int64_t want_blocks, int64_t want_docs) {
    if (want_blocks > m->cap_blocks) {
        const int64_t nb = std::max<int64_t>(want_blocks, m->cap_blocks + m->cap_blocks / 2);
        const size_t blk = (size_t)kMsBlkRows * m->dpad * sizeof(float), blk16 = (size_t)m->nkk * 64 * sizeof(uint4);
        CHECK(ms_regrow(idx, m->tok, nb * blk, m->n_blocks * blk));
        CHECK(ms_regrow(idx, m->tok16, nb * blk16, m->n_blocks * blk16));
        m->cap_blocks = nb;
    }
    if (want_docs > m->cap_docs) {
        const int64_t nd = std::max<int64_t>(want_docs, m->cap_docs + m->cap_docs / 2);
        // (the stored docs' offsets stay valid on the device whatever becomes of the add that asked for the room)
        CHECK(ms_regrow(idx, m->blk_off, (size_t)(nd + 1) * sizeof(int64_t), m->blk_off.p ? (size_t)(m->n_docs + 1) * sizeof(int64_t) : 0));
        m->cap_docs = nd;
    }
    return MI355DR_OK;
}

// A host payload is staged on the device in slices of whole documents of at most this many bytes (a longer document goes
// alone) and built slice by slice: the device memory a call needs beyond the store does not grow with the call.
constexpr size_t kMsAddSliceBytes = (size_t)32 << 20;

// The documents of one call whose images are to be written: the ONE slice loop behind add and set.
struct MsBuild {
    const float* vecs;        // [.., dim] on the host, or (on_device) on the index's GPU, read in place
    const int64_t* offsets;   // [n + 1]: document j owns rows offsets[j] .. offsets[j + 1] of vecs
    int64_t n;
    bool on_device;
    int64_t blk_base;         // add: the documents' blocks follow each other from this block on (k_ms_build) ...
    const int64_t* doc_dst0;  // ... set: [n] the first destination block of every document (k_ms_build_at); nullptr for an add
    float* tok;               // the images that are written into
    uint16_t* tok16;
};

// k_ms_build(_at) per slice of whole docs [i0, i1): a device payload is one slice read in place, a host payload's slices are
// staged.  Every buffer is allocated before the first block is written (an allocation that fails has changed no image), and the
// call is complete on return: st = the three maxima of the built tokens (double bit patterns) and (int) their not-finite flag.
int ms_build_docs(mi355dr_index* idx, const MultiVecStore* m, const MsBuild& j, unsigned long long st[4]) {
    const int d = idx->dim;
    const int64_t* offsets = j.offsets;
    hipStream_t s = idx->stream;
    auto blocks_of = [&](int64_t i) { return (offsets[i + 1] - offsets[i] + kMsBlkRows - 1) / kMsBlkRows; };
    const int64_t slice_rows = j.on_device ? INT64_MAX : std::max<int64_t>(1, (int64_t)(kMsAddSliceBytes / ((size_t)d * sizeof(float))));
    std::vector<int64_t> ends;  // i1 of every slice
    size_t max_bytes = 0, max_docs = 0, max_blocks = 0;
    for (int64_t i0 = 0, i1; i0 < j.n; i0 = i1) {
        int64_t rows = 0, blocks = 0;  // (a doc without vectors counts as one row: the tables of a slice are bounded like its vectors)
        for (i1 = i0; i1 < j.n && (i1 == i0 || rows + std::max<int64_t>(offsets[i1 + 1] - offsets[i1], 1) <= slice_rows); ++i1) {
            rows += std::max<int64_t>(offsets[i1 + 1] - offsets[i1], 1);
            blocks += blocks_of(i1);
        }
        ends.push_back(i1);
        if (blocks == 0) continue;
        max_bytes = std::max(max_bytes, (size_t)(offsets[i1] - offsets[i0]) * d * sizeof(float));
        max_docs = std::max(max_docs, (size_t)(i1 - i0));
        max_blocks = std::max(max_blocks, (size_t)blocks);
    }
    DevBuf<float> stage;
    DevBuf<int64_t> tok0_dev, T_dev, blk0_dev, dst0_dev;
    DevBuf<int32_t> blk_doc_dev;
    DevBuf<unsigned long long> stats;  // [3] the maxima of the build kernels, then (int) their not-finite flag
    HIPCHECK(idx, stats.grow(4 * sizeof(unsigned long long)));
    if (!j.on_device) HIPCHECK(idx, stage.grow(max_bytes));
    HIPCHECK(idx, tok0_dev.grow(max_docs * sizeof(int64_t)));
    HIPCHECK(idx, T_dev.grow(max_docs * sizeof(int64_t)));
    HIPCHECK(idx, blk0_dev.grow(max_docs * sizeof(int64_t)));
    if (j.doc_dst0) HIPCHECK(idx, dst0_dev.grow(max_docs * sizeof(int64_t)));
    HIPCHECK(idx, blk_doc_dev.grow(max_blocks * sizeof(int32_t)));
    HIPCHECK(idx, hipMemsetAsync(stats.p, 0, stats.bytes, s));
    std::vector<int64_t> tok0, T, blk0;  // of the slice's docs: first token in `src`, tokens, first block in the slice
    std::vector<int32_t> blk_doc;        // of the slice's blocks: doc in the slice
    int64_t blk_base = j.blk_base, i0 = 0;
    for (const int64_t i1 : ends) {
        tok0.clear(), T.clear(), blk0.clear(), blk_doc.clear();
        const int64_t t_base = j.on_device ? 0 : offsets[i0];
        for (int64_t i = i0; i < i1; ++i) {
            tok0.push_back(offsets[i] - t_base);
            T.push_back(offsets[i + 1] - offsets[i]);
            blk0.push_back((int64_t)blk_doc.size());
            blk_doc.insert(blk_doc.end(), (size_t)blocks_of(i), (int32_t)(i - i0));
        }
        const int64_t first = i0;
        i0 = i1;
        if (blk_doc.empty()) continue;
        const float* src = j.vecs;
        if (!j.on_device) {
            const size_t bytes = (size_t)(offsets[i1] - offsets[first]) * d * sizeof(float);
            HIPCHECK(idx, hipMemcpyAsync(stage.p, j.vecs + offsets[first] * d, bytes, hipMemcpyHostToDevice, s));
            src = stage.p;
        }
        const size_t nd = (size_t)(i1 - first) * sizeof(int64_t);
        HIPCHECK(idx, hipMemcpyAsync(tok0_dev.p, tok0.data(), nd, hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(T_dev.p, T.data(), nd, hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(blk0_dev.p, blk0.data(), nd, hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(blk_doc_dev.p, blk_doc.data(), blk_doc.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (j.doc_dst0) {
            HIPCHECK(idx, hipMemcpyAsync(dst0_dev.p, j.doc_dst0 + first, nd, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_ms_build_at, dim3((unsigned)blk_doc.size()), dim3(64), 0, s, src, tok0_dev.p, T_dev.p, blk_doc_dev.p,
                               blk0_dev.p, dst0_dev.p, d, m->dpad, m->nkk, j.tok, j.tok16, stats.p, (int*)(stats.p + 3));
        } else {
            hipLaunchKernelGGL(k_ms_build, dim3((unsigned)blk_doc.size()), dim3(64), 0, s, src, tok0_dev.p, T_dev.p, blk_doc_dev.p,
                               blk0_dev.p, d, m->dpad, m->nkk, blk_base, j.tok, j.tok16, stats.p, (int*)(stats.p + 3));
        }
        HIPCHECK(idx, hipGetLastError());
        HIPCHECK(idx, hipStreamSynchronize(s));  // (the host tables and the staging buffer are rewritten for the next slice)
        blk_base += (int64_t)blk_doc.size();
    }
    HIPCHECK(idx, hipMemcpyAsync(st, stats.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    return MI355DR_OK;
}

// the bound quantities only ever move in the conservative direction: the maxima grow, `finite` turns false
void ms_commit_bounds(MultiVecStore* m, const unsigned long long st[4]) {
    double v[3];
    memcpy(v, st, sizeof(v));
    int nf;
    memcpy(&nf, &st[3], sizeof(nf));
    m->tok_norm_max = std::max(m->tok_norm_max, v[0]);
    m->tok16_norm_max = std::max(m->tok16_norm_max, v[1]);
    m->tok_res_max = std::max(m->tok_res_max, v[2]);
    if (nf) m->finite = false;
}

// the index's store, created empty on first use
MultiVecStore* ms_store(mi355dr_index* idx) {
    if (!idx->mv) {
        idx->mv = new MultiVecStore();
        idx->mv->dpad = (int)round_up(idx->dim, 8);
        idx->mv->nkk = (int)round_up(idx->dim, 16) / 16;
        idx->mv->blk_off_host.push_back(0);
    }
    return idx->mv;
}

// vecs: [offsets[n_docs], dim] on the host, or (on_device) on the index's GPU.  All or nothing: room for the whole call is
// reserved first (what is stored is carried over, the device offset table included), the images of the new blocks and the new
// docs' entries of the device offset table are written behind the stored ones (no search reads past n_blocks / n_docs), and
// n_docs, n_blocks, the host offset table, the token counts and the bound maxima change only after every step succeeded.
int ms_add(mi355dr_index* idx, const float* vecs, const int64_t* offsets, int64_t n_docs, bool on_device) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "add_multivec");
    if (n_docs < 0 || !offsets || (n_docs > 0 && offsets[n_docs] > 0 && !vecs))
        return fail(idx, MI355DR_E_INVALID, "bad multi-vector arguments");
    if (n_docs == 0) return MI355DR_OK;
    for (int64_t i = 0; i < n_docs; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(idx, MI355DR_E_INVALID, "offsets must be non-decreasing");
    HIPCHECK(idx, hipSetDevice(idx->device));
    MultiVecStore* m = ms_store(idx);
    if (m->n_docs + n_docs >= ((int64_t)1 << 31)) return fail(idx, MI355DR_E_UNSUPPORTED, "too many docs");
    auto blocks_of = [&](int64_t i) { return (offsets[i + 1] - offsets[i] + kMsBlkRows - 1) / kMsBlkRows; };
    // the table with the new docs' block offsets, built on the side
    std::vector<int64_t> table(m->blk_off_host);
    table.reserve(table.size() + (size_t)n_docs);
    int64_t new_blocks = 0;
    for (int64_t i = 0; i < n_docs; ++i) table.push_back(m->n_blocks + (new_blocks += blocks_of(i)));
    CHECK(ms_reserve(idx, m, m->n_blocks + new_blocks, m->n_docs + n_docs));
    hipStream_t s = idx->stream;
    unsigned long long st[4] = {0, 0, 0, 0};
    CHECK(ms_build_docs(idx, m, MsBuild{vecs, offsets, n_docs, on_device, m->n_blocks, nullptr, m->tok.p, (uint16_t*)m->tok16.p}, st));
    HIPCHECK(idx, hipMemcpyAsync(m->blk_off.p, table.data(), table.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    // ---- commit (nothing below fails; until here a search saw the store as it was: entries past n_docs / n_blocks are not read)
    m->blk_off_host.swap(table);
    ms_commit_bounds(m, st);
    for (int64_t i = 0; i < n_docs; ++i) {
        m->tok_cnt_host.push_back((int32_t)(offsets[i + 1] - offsets[i]));
        m->n_live += offsets[i + 1] > offsets[i] ? 1 : 0;
    }
    m->n_blocks += new_blocks;
    m->n_docs += n_docs;
    return MI355DR_OK;
}

// A set makes the granule-packed copy (tok16p, goff) stale as a whole: its incremental branch knows appended documents only, so
// the next pass that takes it packs it anew (pack_docs = -1) and none reads it before (pack_use).  The stat "maxsim_packed_blocks"
// reads 0 (none built for these contents) until ms_pack8_ensure has packed again -- if it decides not to, it stays 0.  `release`:
// the copy's memory goes too.
void ms_pack8_stale(mi355dr_index* idx, MultiVecStore* m, bool release) {
    m->pack_docs = -1;
    m->pack_use = false;
    m->pack_blocks = 0;
    idx->s_ms_packed_blocks = 0;
    if (!release) return;
    m->tok16p.release();
    m->pack_cap_blocks = 0;
}

// ---- replace / remove documents in place (mi355dr_set_multivec) ----
// Document doc_ids[j] takes the vectors offsets[j] .. offsets[j + 1] (none: the document is removed -- a document without vectors,
// the state every reader already skips).  Two write paths, chosen per call:
//   in place   no touched document changes its block count: its blocks of the live images are rewritten (k_ms_build_at), nothing
//              else is read or written.  O(touched blocks).
//   relayout   some block count changes, so everything behind it shifts: a new cumulative table on the host, FRESH tok / tok16
//              buffers (ms_reserve's capacity policy), the untouched documents' blocks moved by k_ms_relayout (one run per maximal
//              stretch of untouched documents), the touched documents' blocks built from the new vectors, the buffers and the
//              device table swapped at the commit.  One device pass over the store; peak = one extra copy of both images until
//              the call returns.
// All or nothing: arguments are checked before anything is touched, every allocation is made before the first write, and
// n_blocks, both offset tables, the token counts, the maxima and (relayout) the buffers change at a commit that cannot fail.  The
// in-place path writes the touched blocks of the live images before that commit: what can still fail then is a copy or a launch
// on the stream (MI355DR_E_HIP, a broken device), never an allocation.
int ms_set(mi355dr_index* idx, const int64_t* doc_ids, const float* vecs, const int64_t* offsets, int64_t n, bool on_device) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "set_multivec");
    if (n < 0 || (n > 0 && (!doc_ids || !offsets))) return fail(idx, MI355DR_E_INVALID, "bad set_multivec arguments");
    if (n == 0) return MI355DR_OK;
    MultiVecStore* m = idx->mv;
    if (!m || m->n_docs == 0) return fail(idx, MI355DR_E_INVALID, "set_multivec: the index has no multi-vector store");
    for (int64_t j = 0; j < n; ++j)
        if (offsets[j + 1] < offsets[j]) return fail(idx, MI355DR_E_INVALID, "offsets must be non-decreasing");
    if (offsets[n] > offsets[0] && !vecs) return fail(idx, MI355DR_E_INVALID, "null vectors");
    std::vector<int64_t> order((size_t)n);  // the call's documents by ascending id
    for (int64_t j = 0; j < n; ++j) {
        if (doc_ids[j] < 0 || doc_ids[j] >= m->n_docs)
            return fail(idx, MI355DR_E_INVALID, "set_multivec: document id " + std::to_string(doc_ids[j]) + " out of range");
        if (offsets[j + 1] - offsets[j] > INT32_MAX) return fail(idx, MI355DR_E_UNSUPPORTED, "too many vectors in one document");
        order[j] = j;
    }
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return doc_ids[a] < doc_ids[b]; });
    for (int64_t r = 1; r < n; ++r)
        if (doc_ids[order[r]] == doc_ids[order[r - 1]])
            return fail(idx, MI355DR_E_INVALID, "set_multivec: document id " + std::to_string(doc_ids[order[r]]) + " listed twice");
    HIPCHECK(idx, hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    const std::vector<int64_t>& old = m->blk_off_host;
    auto blocks_of = [&](int64_t j) { return (offsets[j + 1] - offsets[j] + kMsBlkRows - 1) / kMsBlkRows; };
    bool in_place = true;
    for (int64_t j = 0; j < n && in_place; ++j) in_place = blocks_of(j) == old[doc_ids[j] + 1] - old[doc_ids[j]];
    std::vector<int64_t> dst0((size_t)n);  // first destination block of every document of the call
    std::vector<int64_t> table;            // relayout: the new cumulative table
    DevBuf<float> tok_new;
    DevBuf<uint4> tok16_new;
    DevBuf<int64_t> blk_off_new;
    int64_t cap_new = m->cap_blocks, moved = 0;
    float* tok_dst = m->tok.p;
    uint4* tok16_dst = m->tok16.p;
    if (in_place) {
        for (int64_t j = 0; j < n; ++j) dst0[j] = old[doc_ids[j]];
        // (stale before the first block of the live images is rewritten: a copy or launch that fails half-way leaves no pass
        // reading a packed copy that no longer matches them)
        ms_pack8_stale(idx, m, false);
    } else {
        // the new table and the runs: documents [prev, t) in front of every touched document t, and those behind the last one
        table.resize(old.size());
        std::vector<MsRun> runs;
        int64_t prev = 0;
        table[0] = 0;
        auto run_to = [&](int64_t t) {  // untouched documents [prev, t): table entries, one run
            const int64_t shift = table[prev] - old[prev];
            for (int64_t i = prev; i < t; ++i) table[i + 1] = old[i + 1] + shift;
            if (old[t] > old[prev]) runs.push_back(MsRun{table[prev], old[prev], old[t] - old[prev]});
            moved += old[t] - old[prev];
        };
        for (int64_t r = 0; r < n; ++r) {
            const int64_t j = order[r], t = doc_ids[j];
            run_to(t);
            dst0[j] = table[t];
            table[t + 1] = table[t] + blocks_of(j);
            prev = t + 1;
        }
        run_to(m->n_docs);
        const int64_t nb = table[m->n_docs];
        if (nb > cap_new) cap_new = std::max<int64_t>(nb, m->cap_blocks + m->cap_blocks / 2);
        cap_new = std::max<int64_t>(cap_new, 1);
        // (the granule-packed copy is stale whatever becomes of this call's images and is packed whole after it: an optional
        // shadow, it goes before the fresh buffers come and never adds to the peak; a call that fails from here on has cost a repack)
        ms_pack8_stale(idx, m, true);
        HIPCHECK(idx, tok_new.grow((size_t)cap_new * kMsBlkRows * m->dpad * sizeof(float)));
        HIPCHECK(idx, tok16_new.grow((size_t)cap_new * m->nkk * 64 * sizeof(uint4)));
        HIPCHECK(idx, blk_off_new.grow((size_t)(m->cap_docs + 1) * sizeof(int64_t)));
        tok_dst = tok_new.p;
        tok16_dst = tok16_new.p;
        DevBuf<MsRun> runs_dev;
        if (!runs.empty()) {
            HIPCHECK(idx, runs_dev.grow(runs.size() * sizeof(MsRun)));
            HIPCHECK(idx, hipMemcpyAsync(runs_dev.p, runs.data(), runs.size() * sizeof(MsRun), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_ms_relayout, dim3((unsigned)((nb + kMsRelayoutWaves - 1) / kMsRelayoutWaves)), dim3(64 * kMsRelayoutWaves),
                               0, s, (const uint4*)m->tok.p, (const uint4*)m->tok16.p, runs_dev.p, (int)runs.size(), nb, m->dpad / 8,
                               m->nkk, (uint4*)tok_new.p, tok16_new.p);
            HIPCHECK(idx, hipGetLastError());
        }
        HIPCHECK(idx, hipMemcpyAsync(blk_off_new.p, table.data(), table.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipStreamSynchronize(s));  // (`runs` and its device copy end with this scope)
    }
    unsigned long long st[4] = {0, 0, 0, 0};
    CHECK(ms_build_docs(idx, m, MsBuild{vecs, offsets, n, on_device, 0, dst0.data(), tok_dst, (uint16_t*)tok16_dst}, st));
    // ---- commit (nothing below fails)
    if (!in_place) {
        m->tok.swap(tok_new);  // (the old images are released when this call returns)
        m->tok16.swap(tok16_new);
        m->blk_off.swap(blk_off_new);
        m->blk_off_host.swap(table);
        m->cap_blocks = cap_new;
        m->n_blocks = m->blk_off_host[m->n_docs];
    }
    ms_commit_bounds(m, st);
    for (int64_t j = 0; j < n; ++j) {
        int32_t& cnt = m->tok_cnt_host[doc_ids[j]];
        const int32_t T = (int32_t)(offsets[j + 1] - offsets[j]);
        m->n_live += (T > 0 ? 1 : 0) - (cnt > 0 ? 1 : 0);
        cnt = T;
    }
    idx->s_ms_set_docs += n;
    idx->s_ms_moved_blocks += moved;
    return MI355DR_OK;
}

// ---- the granule-packed bf16 copy (k_maxsim_wg8.h) ----
// Makes the packed copy current for the store's docs, or decides it is not to be used (m->pack_use).  Called with the index lock
// held, before a screen launch on stream `s` that could take it.  A failed allocation is not an error: the padded copy serves.
int ms_pack8_ensure(mi355dr_index* idx, MultiVecStore* m, hipStream_t s) {
    if (m->pack_docs == m->n_docs && (m->pack_use || m->pack_mode == idx->maxsim_pack8)) return MI355DR_OK;
    // a store that grew since the copy was built is packed from the block its new granules start in (an ingest loop that searches
    // between its adds pays for the new documents only); a copy that was never built, was judged not to pay, or must move is
    // packed whole
    int64_t first_block = m->pack_use && m->pack_docs >= 0 && m->pack_docs < m->n_docs ? m->pack_gran / 4 : 0;
    m->pack_docs = m->n_docs;
    m->pack_mode = idx->maxsim_pack8;
    m->pack_use = false;
    if (m->nkk != 8 || (int64_t)m->tok_cnt_host.size() != m->n_docs || m->n_blocks == 0) return MI355DR_OK;
    std::vector<int64_t> goff((size_t)m->n_docs + 1);
    goff[0] = 0;
    for (int64_t i = 0; i < m->n_docs; ++i) goff[i + 1] = goff[i] + (m->tok_cnt_host[i] + 7) / 8;
    const int64_t n_gran = goff[m->n_docs], n_pb = (n_gran + 3) / 4;
    if (n_gran == 0) return MI355DR_OK;
    if (idx->maxsim_pack8 < 0 && (double)n_pb > 0.95 * (double)m->n_blocks) return MI355DR_OK;  // (long documents: nothing to gain)
    if (n_pb > m->pack_cap_blocks) {  // (an optional copy: the old block goes first, it never costs the store its peak)
        first_block = 0;
        m->tok16p.release();
        m->pack_cap_blocks = 0;
        const int64_t want = std::max<int64_t>(n_pb, std::min<int64_t>(m->cap_blocks, n_pb + n_pb / 2));
        if (m->tok16p.grow((size_t)want * m->nkk * 64 * sizeof(uint4)) != hipSuccess) {
            (void)hipGetLastError();
            return MI355DR_OK;
        }
        m->pack_cap_blocks = want;
    }
    if (m->n_docs > m->pack_cap_docs) {
        m->goff.release();
        m->pack_cap_docs = 0;
        if (m->goff.grow((size_t)(m->cap_docs + 1) * sizeof(int64_t)) != hipSuccess) {
            (void)hipGetLastError();
            return MI355DR_OK;
        }
        m->pack_cap_docs = m->cap_docs;
    }
    DevBuf<int32_t> cnt;
    if (cnt.grow((size_t)m->n_docs * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return MI355DR_OK;
    }
    HIPCHECK(idx, hipMemcpyAsync(cnt.p, m->tok_cnt_host.data(), (size_t)m->n_docs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipMemcpyAsync(m->goff.p, goff.data(), goff.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (n_pb > first_block) {  // (new documents without vectors add no granule)
        hipLaunchKernelGGL(k_ms_pack8, dim3((unsigned)(n_pb - first_block)), dim3(64), 0, s, m->tok16.p, m->blk_off.p, cnt.p, m->goff.p,
                           m->n_docs, n_gran, m->nkk, m->tok16p.p, first_block);
        HIPCHECK(idx, hipGetLastError());
        idx->s_ms_packed_built += n_pb - first_block;
    }
    HIPCHECK(idx, hipStreamSynchronize(s));  // (the host vectors above are the copies' sources)
    m->pack_gran = n_gran;
    m->pack_blocks = n_pb;
    m->pack_use = true;
    idx->s_ms_packed_blocks = n_pb;
    return MI355DR_OK;
}

// ---- the search -----------------------------------------------------------------------------------------------------------------
// Round 4: a PASS = up to kMsPassGroups groups of <= 4 queries (dims <= 128, k <= kMsFastK): one screen launch for all of them,
// then ONE selection / candidate / exact re-score / final sequence for all of them (grid.y = query of the pass) and one host
// synchronisation -- rounds 2-3 ran that sequence (ten launches, three copies, one synchronisation) once per group of four.

constexpr int kPQ = kMsPassQueries;
// columns of the fp32 query image of a pass: every group's columns behind the previous group's (+ 32 columns of slack: the
// list form of k_maxsim stages whole 32-column blocks from a query's FIRST column on; those columns' results are never read)
constexpr int kMsImgCols = kMsPassBlocks * 32 + 32;

// what one search call fixes for all of its passes (ms_search_prepare)
struct MsSearch {
    mi355dr_index* idx;
    MultiVecStore* m;
    hipStream_t s;
    const float* qtok;  // HOST [sum_nq, dim]
    const int32_t* q_offsets;
    int B, k;
    float* out_dist;
    int64_t* out_rows;
    bool out_dev;
    int cols;           // query vectors one launch of the EXACT kernel stages; longer queries are scored in tiles
    size_t lds, lds16;  // dynamic LDS of a full-scan launch of k_maxsim / of the generic screen
    int seg;            // ms_topk's segment size
    unsigned grid_all;  // k_maxsim over every doc
    int64_t n_cand_max;
    double eps;
    // the pinned staging area (pageable copies are synchronous and cost ~20 us each): query image | query fragments | hd | hr.
    // hd stages 2E on its way up, then receives the result distances; hr the result rows.
    size_t qimg_n, qf16_n;
    float* qimg;
    uint16_t* qf16;
    float* hd;
    int64_t* hr;
    MsArgs a0;  // k_maxsim over every doc of the store (a subset search: over its list), query image at m->qtok.p: the launches below start from it
    // ---- a search within a listed subset (mi355dr_search_maxsim_subset; nullptr: every document).  The "full scan" of such a
    // search walks the list, its screen is the list form, and the selection kernels read `has_vec` where they read blk_off.
    const int32_t* list;     // DEVICE [n_list] documents with vectors: local, ascending, unique
    int64_t n_list;
    bool list_screen;        // option maxsim_subset_screen, resolved for this list
    int64_t scan_n;          // items of a full scan: n_list, or n_docs
    unsigned grid_scan;
    const int64_t* has_vec;  // [n_docs + 1] table with t[d + 1] > t[d] for the documents a dense pass may look at: blk_off, or the membership table
};

// (the stats and the profile of mi355dr_search_maxsim do not move for a subset search)
inline bool ms_prof(const MsSearch& c) { return c.idx->profile && !c.list; }

// one group = up to 4 queries whose token counts fit `cols` columns (packed tightly: a query may start anywhere in a column block)
struct MsGroup {
    int nql = 0, col = 0, b_end = 0;
    int q_col0[4] = {0, 0, 0, 0}, q_len[4] = {0, 0, 0, 0};
    double two_e[4] = {0, 0, 0, 0};
    bool finite = true;
};

// a pass: its LIVE queries (a query without vectors: reference `if not query_vectors: return []`) -- row r of the screen
// distances, of the candidate lists, of the results
struct MsPass {
    int n = 0;                        // live queries
    int b[kPQ], col0[kPQ], len[kPQ];  // query of the call, first column in the pass's images, vectors
    double two_e[kPQ];
    int total_col = 0;                // columns of the pass's images in use
    bool screen = false;              // bf16 screen + re-score; else the exact kernel over every doc (first group only)
    int first = 0, b_end = 0;         // queries [first, b_end) of the call
    MsGroup g0;                       // the first group, as packed (its empty queries included)
};

// sums over the vectors of one query, for its bound
struct MsQueryNorms {
    double norm_sum = 0.0, res_sum = 0.0;  // of |q_i| / of the bf16 residuals |q_i - bf16(q_i)|
    bool finite = true;
};

// one query vector: its bf16 fragment at column cc of qf16 (nullptr: none) and its share of the query's norms.
// block cb = column / 32, lane = (column & 31) + 32 * half
void ms_pack_frag(const float* sv, int d, int nkk, int cc, uint16_t* qf16, MsQueryNorms& qn) {
    double n2 = 0.0, r2 = 0.0;
    for (int c = 0; c < d; ++c) {
        if (!std::isfinite(sv[c])) qn.finite = false;
        const uint16_t h = host_bf16_rn(sv[c]);
        const double x = sv[c], x16 = host_bf16_to_f32(h);
        n2 += x * x;
        r2 += (x - x16) * (x - x16);
        if (qf16) {
            const int kk = c / 16, half = (c % 16) / 8, jj = c % 8;
            qf16[((((size_t)(cc >> 5) * nkk + kk) * 64) + (cc & 31) + 32 * half) * 8 + jj] = h;
        }
    }
    qn.norm_sum += std::sqrt(n2);
    qn.res_sum += std::sqrt(r2);
}

// 2E of a query of nq vectors
double ms_two_e(const MultiVecStore* m, int d, int nq, double eps, const MsQueryNorms& qn) {
    // per token pair: |q16.d16 - q.d| <= |r_q||d16| + |q||r_d| with the residuals MEASURED (round-to-nearest leaves
    // about half of the a-priori 2^-8 |x|), + fp32 accumulation of both dot products and of the per-doc sums
    const double e_pair = qn.res_sum * m->tok16_norm_max + qn.norm_sum * m->tok_res_max;
    const double e_acc = (3.0 * d + 2.0 * nq) * std::ldexp(1.0, -24) * m->tok_norm_max * qn.norm_sum;
    return 2.0 * std::min(e_pair + e_acc, (eps + 2.0 * nq * std::ldexp(1.0, -24)) * m->tok_norm_max * qn.norm_sum) * (1.0 + 1e-6);
}

// the group that starts at query b0: its bf16 fragments at column base `fcol0` of qf16 (fcol0 < 0: none) and its fp32
// image for the exact kernel at column base `icol0` of qimg (icol0 < 0: none)
MsGroup ms_pack_group(const MsSearch& c, int b0, int fcol0, int icol0) {
    const int d = c.idx->dim, dp = c.m->dpad;
    MsGroup g;
    int bb = b0;
    while (bb < c.B && g.nql < 4) {
        const int nq = c.q_offsets[bb + 1] - c.q_offsets[bb];
        const int need = std::max(nq, 1);  // (columns are packed tightly: no padding of a query to whole 32-column blocks)
        if (g.col + need > c.cols) break;  // (a query longer than `cols` never fits: the caller scores it in tiles)
        g.q_col0[g.nql] = g.col;
        g.q_len[g.nql] = nq;
        MsQueryNorms qn;
        for (int j = 0; j < nq; ++j) {
            const float* sv = c.qtok + (int64_t)(c.q_offsets[bb] + j) * d;
            if (icol0 >= 0) multivec_pack_query_row(sv, d, dp, &c.qimg[(size_t)(icol0 + g.col + j) * dp]);
            ms_pack_frag(sv, d, c.m->nkk, fcol0 + g.col + j, fcol0 >= 0 ? c.qf16 : nullptr, qn);
        }
        if (!qn.finite) g.finite = false;
        g.two_e[g.nql] = ms_two_e(c.m, d, nq, c.eps, qn);
        g.col += need;
        ++g.nql;
        ++bb;
    }
    g.b_end = bb;
    return g;
}

// scratch, function attributes, staging, the call's constants.  c.idx ... c.out_dev are set by the caller.
int ms_search_prepare(MsSearch& c) {
    mi355dr_index* idx = c.idx;
    MultiVecStore* m = c.m;
    const int dp = m->dpad, nkk = m->nkk;
    c.cols = ms_cols_for(dp);
    if (c.cols < 32) return fail(idx, MI355DR_E_UNSUPPORTED, "dim too large for the MaxSim kernel's LDS budget (dim <= 1272)");
    c.lds = (size_t)c.cols * (dp + 4) * sizeof(float);
    c.lds16 = (size_t)4 * nkk * 64 * sizeof(uint4);
    if (!m->scratch_ready) {  // (a failed attempt keeps what it got: grow() finds it there the next time)
        HIPCHECK(idx, m->qtok.grow((size_t)kMsImgCols * dp * sizeof(float)));
        HIPCHECK(idx, hipMemsetAsync(m->qtok.p, 0, (size_t)kMsImgCols * dp * sizeof(float), c.s));
        HIPCHECK(idx, m->qfrag.grow(kMsPassGroups * c.lds16));
        HIPCHECK(idx, m->out_d.grow((size_t)kPQ * kKMax * sizeof(float)));
        HIPCHECK(idx, m->out_r.grow((size_t)kPQ * kKMax * sizeof(int64_t)));
        HIPCHECK(idx, m->cand_list.grow((size_t)3 * kPQ * kMsCandCap * sizeof(int32_t)));
        HIPCHECK(idx, m->cand_dist.grow((size_t)kPQ * kMsCandCap * sizeof(float)));
        HIPCHECK(idx, m->cand_sd.grow((size_t)kPQ * kMsCandCap * sizeof(float)));
        HIPCHECK(idx, m->cand_ctl.grow(3 * 2 * kPQ * sizeof(int)));
        HIPCHECK(idx, m->two_e_dev.grow(kPQ * sizeof(float)));
        HIPCHECK(idx, m->cand_ctl_host.grow(2 * kPQ * sizeof(int)));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_ms_final, hipFuncAttributeMaxDynamicSharedMemorySize, kMsCandCap * 12));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_maxsim, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(c.lds + kMsRedBytes)));
        CHECK(ms16_prepare(idx, c.lds16));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_topk_segments, hipFuncAttributeMaxDynamicSharedMemorySize, kSegSort * 12));
        m->scratch_ready = true;
    }
    HIPCHECK(idx, m->dist.grow((size_t)4 * m->cap_docs * sizeof(float)));
    HIPCHECK(idx, m->dist16.grow((size_t)kPQ * m->cap_docs * sizeof(float)));
    for (auto& b : m->sel) HIPCHECK(idx, b.grow((size_t)kPQ * ((m->cap_docs + kMsSelSeg - 1) / kMsSelSeg) * kMsFastK * sizeof(uint32_t)));
    // segment size: small segments = many workgroups; it must hold k and shrink the list by >= 4x per stage.p
    c.seg = 512;
    while (c.seg < 4 * c.k) c.seg <<= 1;
    if (c.seg > kSegSort) c.seg = kSegSort;
    const int64_t nseg0 = (m->n_docs + c.seg - 1) / c.seg;
    for (auto& b : m->pk) HIPCHECK(idx, b.grow((size_t)nseg0 * kKMax * sizeof(uint64_t)));
    for (auto& b : m->pr) HIPCHECK(idx, b.grow((size_t)nseg0 * kKMax * sizeof(int32_t)));
    c.grid_all = (unsigned)((m->n_docs + 4 * kMsDocsPerWave - 1) / (4 * kMsDocsPerWave));
    c.scan_n = c.list ? c.n_list : m->n_docs;
    // (a list launch of k_maxsim strides over its items: two workgroups per CU)
    c.grid_scan = c.list ? (unsigned)std::min<int64_t>((c.n_list + 3) / 4, 2 * kMsListGrid) : c.grid_all;
    c.has_vec = c.list ? m->sub_memb.p : m->blk_off.p;
    c.n_cand_max = std::min<int64_t>(kMsCandCap, m->n_docs);
    // bf16 round-to-nearest: unit roundoff 2^-8 per operand -> 2^-7 + 2^-16 per product
    c.eps = std::ldexp(1.0, -7) + std::ldexp(1.0, -15) + 3.0 * idx->dim * std::ldexp(1.0, -24);
    c.qimg_n = (size_t)kMsImgCols * dp;
    c.qf16_n = (size_t)kMsPassBlocks * nkk * 64 * 8;
    HIPCHECK(idx, m->stage_host.grow(c.qimg_n * 4 + c.qf16_n * 2 + (size_t)kPQ * kKMax * 12 + 256));
    c.qimg = (float*)m->stage_host.p;
    c.qf16 = (uint16_t*)(m->stage_host.p + c.qimg_n * 4);
    c.hd = (float*)(m->stage_host.p + c.qimg_n * 4 + c.qf16_n * 2);
    c.hr = (int64_t*)(c.hd + (size_t)kPQ * kKMax + 16);
    c.a0 = MsArgs{};
    c.a0.tok = m->tok.p;
    c.a0.blk_off = m->blk_off.p;
    c.a0.qtok = m->qtok.p;
    c.a0.dist = m->dist.p;
    c.a0.n_docs = m->n_docs;
    c.a0.doc_list = c.list;
    c.a0.n_items = c.scan_n;
    c.a0.dpad = dp;
    return MI355DR_OK;
}

// segment-wise top-k of n_in distances (first stage.p) until one segment is left; returns the buffer index holding it
int ms_topk(const MsSearch& c, const float* dist, int64_t n_in, const int32_t* row_map, const int* n_in_dev, int* cur_out) {
    MultiVecStore* m = c.m;
    int cur = 0;
    bool first_stage = true;
    while (true) {
        const int64_t nseg = (n_in + c.seg - 1) / c.seg;
        hipLaunchKernelGGL(k_topk_segments, dim3((unsigned)nseg), dim3(256), (size_t)kSegSort * 12, c.s,
                           first_stage ? dist : nullptr, row_map ? m->blk_off.p : c.has_vec, first_stage ? nullptr : m->pk[cur ^ 1].p,
                           first_stage ? nullptr : m->pr[cur ^ 1].p, n_in, c.k, c.seg, m->pk[cur].p, m->pr[cur].p,
                           first_stage ? row_map : nullptr, first_stage ? n_in_dev : nullptr);
        HIPCHECK(c.idx, hipGetLastError());
        first_stage = false;
        if (nseg == 1) break;
        n_in = nseg * c.k;
        cur ^= 1;
    }
    *cur_out = cur;
    return MI355DR_OK;
}

// the top-k in m->pk / pr [cur] -> the outputs of query b of the call (copies are enqueued, not waited for)
int ms_emit_result(const MsSearch& c, int cur, int b) {
    mi355dr_index* idx = c.idx;
    MultiVecStore* m = c.m;
    float* od = c.out_dist + (int64_t)b * c.k;
    int64_t* orow = c.out_rows + (int64_t)b * c.k;
    // (device outputs: straight into the caller's buffers)
    hipLaunchKernelGGL(k_ms_write_out, dim3((c.k + 255) / 256), dim3(256), 0, c.s, m->pk[cur].p, m->pr[cur].p, c.k, idx->row_offset,
                       idx->view_doc_map.p, c.out_dev ? od : m->out_d.p, c.out_dev ? orow : m->out_r.p);
    HIPCHECK(idx, hipGetLastError());
    if (c.out_dev) return MI355DR_OK;
    HIPCHECK(idx, hipMemcpyAsync(od, m->out_d.p, c.k * sizeof(float), hipMemcpyDeviceToHost, c.s));
    HIPCHECK(idx, hipMemcpyAsync(orow, m->out_r.p, c.k * sizeof(int64_t), hipMemcpyDeviceToHost, c.s));
    return MI355DR_OK;
}

// exact kernel over EVERY doc (a subset search: every listed doc) for one query whose image sits at column c0 of m->qtok.p
// -> m->dist.p row 0 -> top-k -> outputs
int ms_full_scan_query(const MsSearch& c, int c0, int len, int b) {
    MsArgs f = c.a0;
    f.qtok = c.m->qtok.p + (int64_t)c0 * c.m->dpad;
    f.nq_launch = 1;
    f.q_col0[0] = 0;
    f.q_len[0] = len;
    hipLaunchKernelGGL(k_maxsim, dim3(c.grid_scan), dim3(kMsThreads), c.lds, c.s, f);
    HIPCHECK(c.idx, hipGetLastError());
    int cur = 0;
    CHECK(ms_topk(c, c.m->dist.p, c.scan_n, c.list, nullptr, &cur));
    CHECK(ms_emit_result(c, cur, b));
    HIPCHECK(c.idx, hipStreamSynchronize(c.s));
    if (c.list) c.idx->s_mss_exact++;
    return MI355DR_OK;
}

// ---- a query with more vectors than one launch stages (VectorChord's `@#` has no such limit: base.py:518-524):
// the exact kernel over every doc, one launch per tile of <= cols query vectors, each continuing the per-doc sums
int ms_run_long_query(const MsSearch& c, int b) {
    mi355dr_index* idx = c.idx;
    MultiVecStore* m = c.m;
    const int d = idx->dim, dp = m->dpad, cols = c.cols;
    const int nq = c.q_offsets[b + 1] - c.q_offsets[b];
    for (int t0 = 0; t0 < nq; t0 += cols) {
        const int tl = std::min(cols, nq - t0);
        if (t0 > 0) HIPCHECK(idx, hipStreamSynchronize(c.s));  // (the previous tile's launch has read the staging image)
        std::fill(c.qimg, c.qimg + (size_t)cols * dp, 0.0f);
        for (int j = 0; j < tl; ++j)
            multivec_pack_query_row(c.qtok + (int64_t)(c.q_offsets[b] + t0 + j) * d, d, dp, &c.qimg[(size_t)j * dp]);
        HIPCHECK(idx, hipMemcpyAsync(m->qtok.p, c.qimg, (size_t)cols * dp * sizeof(float), hipMemcpyHostToDevice, c.s));
        MsArgs f = c.a0;
        f.nq_launch = 1;
        f.q_col0[0] = 0;
        f.q_len[0] = tl;
        f.dist_in = t0 > 0 ? m->dist.p : nullptr;
        hipLaunchKernelGGL(k_maxsim, dim3(c.grid_scan), dim3(kMsThreads), c.lds, c.s, f);
        HIPCHECK(idx, hipGetLastError());
    }
    (c.list ? idx->s_mss_exact : idx->s_ms_fallbacks)++;
    int cur = 0;
    CHECK(ms_topk(c, m->dist.p, c.scan_n, c.list, nullptr, &cur));
    CHECK(ms_emit_result(c, cur, b));
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    return MI355DR_OK;
}

// ---- the groups of the pass that starts at query b: packs them into the staging images, lists the pass's live queries
MsPass ms_plan_pass(const MsSearch& c, int b) {
    mi355dr_index* idx = c.idx;
    const MultiVecStore* m = c.m;
    const auto t_pack0 = std::chrono::steady_clock::now();
    std::fill(c.qimg, c.qimg + c.qimg_n, 0.0f);
    std::fill(c.qf16, c.qf16 + c.qf16_n, (uint16_t)0);
    MsPass p;
    p.first = b;
    MsGroup gs[kMsPassGroups];
    int gbase[kMsPassGroups] = {0, 0, 0, 0}, gfirst[kMsPassGroups] = {b, 0, 0, 0};
    gs[0] = ms_pack_group(c, b, 0, 0);
    int n_acc = 1, bn = gs[0].b_end;
    p.total_col = gs[0].col;
    p.screen = (c.list ? c.list_screen : idx->maxsim_screen != 0) && m->finite && gs[0].finite && c.lds16 <= 160 * 1024;
    if (p.screen && m->nkk == 8 && c.k <= kMsFastK) {
        // The NEXT groups ride the same pass over the token stream (dims <= 128, the single-launch selection path): their
        // columns packed behind the previous group's
        while (n_acc < kMsPassGroups && n_acc < idx->maxsim_pass_groups && bn < c.B &&
               c.q_offsets[bn + 1] - c.q_offsets[bn] <= c.cols) {
            const MsGroup H = ms_pack_group(c, bn, p.total_col, p.total_col);
            if (H.nql == 0 || !H.finite) {
                // (what the packer may have written for H is not used: rebuild the accepted groups alone)
                std::fill(c.qimg, c.qimg + c.qimg_n, 0.0f);
                std::fill(c.qf16, c.qf16 + c.qf16_n, (uint16_t)0);
                for (int g2 = 0; g2 < n_acc; ++g2) (void)ms_pack_group(c, gfirst[g2], gbase[g2], gbase[g2]);
                break;
            }
            gs[n_acc] = H;
            gbase[n_acc] = p.total_col;
            gfirst[n_acc] = bn;
            p.total_col += H.col;
            bn = H.b_end;
            ++n_acc;
        }
    }
    p.b_end = bn;
    p.g0 = gs[0];
    for (int g = 0; g < n_acc; ++g)
        for (int qi = 0; qi < gs[g].nql; ++qi) {
            if (gs[g].q_len[qi] == 0) continue;
            p.b[p.n] = gfirst[g] + qi;
            p.col0[p.n] = gbase[g] + gs[g].q_col0[qi];
            p.len[p.n] = gs[g].q_len[qi];
            p.two_e[p.n] = gs[g].two_e[qi];
            ++p.n;
        }
    if (p.n > 0 && ms_prof(c))
        idx->s_ms_pack_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_pack0).count();
    return p;
}

// ---- no screen: the exact kernel over every doc (a subset search: over the list) for the whole first group (one launch, <= 4 queries), then a top-k per query
int ms_run_exact_group(const MsSearch& c, const MsPass& p) {
    MultiVecStore* m = c.m;
    MsArgs a = c.a0;
    a.nq_launch = p.g0.nql;
    for (int qi = 0; qi < 4; ++qi) {
        a.q_col0[qi] = p.g0.q_col0[qi];
        a.q_len[qi] = p.g0.q_len[qi];
    }
    hipLaunchKernelGGL(k_maxsim, dim3(c.grid_scan), dim3(kMsThreads), c.lds, c.s, a);
    HIPCHECK(c.idx, hipGetLastError());
    for (int qi = 0; qi < p.g0.nql; ++qi) {
        if (p.g0.q_len[qi] == 0) continue;
        int cur = 0;
        CHECK(ms_topk(c, m->dist.p + (int64_t)qi * c.scan_n, c.scan_n, c.list, nullptr, &cur));
        CHECK(ms_emit_result(c, cur, p.first + qi));
        HIPCHECK(c.idx, hipStreamSynchronize(c.s));
        if (c.list) c.idx->s_mss_exact++;
    }
    return MI355DR_OK;
}

// ---- the screen: one launch for every live query of the pass
int ms_launch_screen(const MsSearch& c, const MsPass& p) {
    mi355dr_index* idx = c.idx;
    MultiVecStore* m = c.m;
    hipStream_t s = c.s;
    const int nkk = m->nkk;
    Ms16Args sa{};
    sa.tok16 = m->tok16.p;
    sa.blk_off = m->blk_off.p;
    sa.qfrag = m->qfrag.p;
    sa.dist = m->dist16.p;
    sa.n_docs = m->n_docs;
    sa.nkk = nkk;
    sa.nq_launch = p.n;
    sa.aligned = idx->maxsim_aligned ? 1 : 0;
    sa.list = c.list;
    sa.n_list = c.n_list;
    for (int r = 0; r < p.n; ++r) {
        sa.q_col0[r] = p.col0[r];
        sa.q_len[r] = p.len[r];
        if (p.col0[r] != 32 * r || p.len[r] > 32) sa.aligned = 0;
    }
    const int ncb_launch = (p.total_col + 31) / 32;
    HIPCHECK(idx, hipMemcpyAsync(m->qfrag.p, c.qf16, (size_t)std::max(ncb_launch, 4) * nkk * 64 * 8 * sizeof(uint16_t),
                                 hipMemcpyHostToDevice, s));
    if (ms_prof(c)) {
        for (auto& e : idx->ms_ev)
            HIPCHECK(idx, e.create());
        HIPCHECK(idx, hipEventRecord(idx->ms_ev[0], s));
    }
    if (c.list) {  // the listed documents where they lie: one wave per document, the padded copy
        CHECK(ms16_list_launch(idx, s, ncb_launch, c.lds16, sa));
    } else if (nkk == 8) {  // dims <= 128: the compile-time-unrolled forms, only as many column blocks as the pass has
        Ms16Pack pk{};
        bool packed = false;
        // the granule-packed copy serves the workgroup form's aligned passes (k_maxsim_wg8.h) and the passes of up to four column
        // blocks (k_maxsim16_d128<.., PK>: one to four queries per call are bound by the token stream's bytes: 10 % fewer)
        const bool wg_form = ms16_takes_wg(idx, ncb_launch, m->n_docs, m->n_blocks);
        if (idx->maxsim_pack8 != 0 && (wg_form ? sa.aligned != 0 : ncb_launch <= 4)) {
            CHECK(ms_pack8_ensure(idx, m, s));
            if (m->pack_use) {
                pk.tok16p = m->tok16p.p;
                pk.goff = m->goff.p;
                pk.n_gran = m->pack_gran;
                pk.n_pblocks = m->pack_blocks;
                packed = true;
            }
        }
        idx->s_ms_packed_launches += packed ? 1 : 0;
        CHECK(ms16_d128_launch(idx, s, ncb_launch, m->n_docs, m->n_blocks, idx->maxsim_persistent != 0, sa, packed ? &pk : nullptr));
    } else {
        CHECK(ms16_generic_launch(idx, s, c.grid_all, c.lds16, sa));
    }
    if (!c.list) idx->s_ms_screen_cols += 32 * (int64_t)ncb_launch;
    if (ms_prof(c)) HIPCHECK(idx, hipEventRecord(idx->ms_ev[1], s));
    return MI355DR_OK;
}

// option "profile", after a host synchronisation: the HIP-event time of the pass's screen launch and (exact) of its re-score launches
void ms_read_profile(mi355dr_index* idx, bool exact) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, idx->ms_ev[0], idx->ms_ev[1]) == hipSuccess) {
        idx->s_ms_screen_ns += (int64_t)(ms * 1e6);
        idx->s_ms_screen_launches++;
    }
    if (exact && hipEventElapsedTime(&ms, idx->ms_ev[2], idx->ms_ev[3]) == hipSuccess) {
        idx->s_ms_exact_ns += (int64_t)(ms * 1e6);
        idx->s_ms_exact_launches++;
    }
}

// k best screen distances of every query of the pass per 1024-entry segment, until one segment is left: m->sel[returned index].p
int ms_select_kth(const MsSearch& c, const MsPass& p, int64_t sel_stride, int* cur_out) {
    MultiVecStore* m = c.m;
    int64_t n_in = m->n_docs;
    int cur = 0;
    bool first_stage = true;
    while (true) {
        const int64_t nseg = (n_in + kMsSelSeg - 1) / kMsSelSeg;
        hipLaunchKernelGGL(k_ms_select, dim3((unsigned)nseg, p.n), dim3(kWave), 0, c.s,
                           first_stage ? m->dist16.p : nullptr, c.has_vec, first_stage ? nullptr : m->sel[cur ^ 1].p, n_in,
                           first_stage ? m->n_docs : sel_stride, c.k, m->sel[cur].p, sel_stride);
        HIPCHECK(c.idx, hipGetLastError());
        first_stage = false;
        if (nseg == 1) break;
        n_in = nseg * c.k;
        cur ^= 1;
    }
    *cur_out = cur;
    return MI355DR_OK;
}

// ---- fast path (k <= kMsFastK): every step handles all queries of the pass at once (grid.y), one host sync per pass.
// handled[r]: query r of the pass has its result (else its candidate list overflowed: the caller's exact full scan)
int ms_fast_path(const MsSearch& c, const MsPass& p, bool* handled) {
    mi355dr_index* idx = c.idx;
    MultiVecStore* m = c.m;
    hipStream_t s = c.s;
    const int k = c.k;
    const int64_t sel_stride = ((m->cap_docs + kMsSelSeg - 1) / kMsSelSeg) * kMsFastK;
    int cur = 0;
    CHECK(ms_select_kth(c, p, sel_stride, &cur));
    float* const te = c.hd;  // (staging: pinned; the results overwrite it after the synchronisation below)
    for (int r = 0; r < p.n; ++r) {
        te[r] = (float)p.two_e[r];
        if ((double)te[r] < p.two_e[r]) te[r] = std::nextafter(te[r], INFINITY);
    }
    HIPCHECK(idx, hipMemcpyAsync(m->two_e_dev.p, te, p.n * sizeof(float), hipMemcpyHostToDevice, s));
    // wide list (+ starter) -> [starter re-scored exactly -> final list] -> final list re-scored exactly -> exact top-k
    const bool tighten = idx->maxsim_tighten != 0;
    int32_t* const list_c = m->cand_list.p;
    int32_t* const list_a = m->cand_list.p + (size_t)kPQ * kMsCandCap;
    int32_t* const list_b = m->cand_list.p + (size_t)2 * kPQ * kMsCandCap;
    int* const ctl_c = m->cand_ctl.p;
    int* const ctl_a = m->cand_ctl.p + 2 * kPQ;
    int* const ctl_b = m->cand_ctl.p + 4 * kPQ;
    HIPCHECK(idx, hipMemsetAsync(m->cand_ctl.p, 0, 3 * 2 * kPQ * sizeof(int), s));
    hipLaunchKernelGGL(k_ms_candidates_y, dim3((unsigned)((m->n_docs + 256 * kMsCandPerThread - 1) / (256 * kMsCandPerThread)), p.n),
                       dim3(256), 0, s, m->dist16.p,
                       m->n_docs, c.has_vec, m->n_docs, m->sel[cur].p, sel_stride, k, m->two_e_dev.p, list_c, kMsCandCap, ctl_c,
                       tighten ? m->cand_sd.p : nullptr, tighten ? list_a : nullptr, tighten ? ctl_a : nullptr);
    HIPCHECK(idx, hipGetLastError());
    MsArgs a = c.a0;  // (the candidate lists replace a subset search's own list; blk_off stays the store's)
    a.dist = m->cand_dist.p;
    a.n_items = c.n_cand_max;
    a.list_stride = kMsCandCap;
    a.nq_launch = p.n;
    for (int r = 0; r < p.n; ++r) {
        a.q_col0[r] = p.col0[r];
        a.q_len[r] = p.len[r];
    }
    // long documents (>= 8 blocks on average: pages): one workgroup per candidate, its four waves share the blocks
    const bool coop = idx->maxsim_coop < 0 ? m->n_blocks >= 8 * m->n_docs : idx->maxsim_coop != 0;
    a.coop = coop ? 1 : 0;
    // LDS for the column blocks the longest query of the pass has (a workgroup stages ONE query's columns), and grids sized
    // for the lists that are usual (the workgroups stride over a list until it ends): 256 x 16 workgroups of 68 KiB each,
    // nearly all of which find nothing to do, cost more than the re-scoring itself
    int len_max = 1;
    for (int r = 0; r < p.n; ++r) len_max = std::max(len_max, p.len[r]);
    const size_t lds_list = (size_t)((len_max + 31) / 32) * 32 * (m->dpad + 4) * sizeof(float);
    a.red_off = (int)lds_list;
    const int64_t want_a = k + 8, want_f = tighten ? 256 : c.n_cand_max;  // documents a launch should cover in ONE round
    const dim3 grid_a((unsigned)std::min<int64_t>({coop ? want_a : (want_a + 3) / 4, c.n_cand_max, (int64_t)kMsListGrid}), p.n);
    const dim3 list_grid((unsigned)std::min<int64_t>({coop ? want_f : (want_f + 3) / 4, c.n_cand_max, (int64_t)kMsListGrid}), p.n);
    if (ms_prof(c)) HIPCHECK(idx, hipEventRecord(idx->ms_ev[2], s));
    const int32_t* list_f = list_c;
    const int* ctl_f = ctl_c;
    if (tighten) {
        a.doc_list = list_a;
        a.n_items_dev = ctl_a;
        hipLaunchKernelGGL(k_maxsim, grid_a, dim3(kMsThreads), lds_list + kMsRedBytes, s, a);
        HIPCHECK(idx, hipGetLastError());
        hipLaunchKernelGGL(k_ms_tighten, dim3(1, p.n), dim3(256), 0, s, m->cand_dist.p, ctl_a, list_c, m->cand_sd.p, ctl_c,
                           kMsCandCap, k, m->two_e_dev.p, list_b, ctl_b);
        HIPCHECK(idx, hipGetLastError());
        list_f = list_b;
        ctl_f = ctl_b;
    }
    a.doc_list = list_f;
    a.n_items_dev = ctl_f;
    hipLaunchKernelGGL(k_maxsim, list_grid, dim3(kMsThreads), lds_list + kMsRedBytes, s, a);
    HIPCHECK(idx, hipGetLastError());
    if (ms_prof(c)) HIPCHECK(idx, hipEventRecord(idx->ms_ev[3], s));
    hipLaunchKernelGGL(k_ms_final, dim3(1, p.n), dim3(256), (size_t)kMsCandCap * 12, s, m->cand_dist.p, list_f, ctl_f,
                       kMsCandCap, k, idx->row_offset, idx->view_doc_map.p, m->out_d.p, m->out_r.p);
    HIPCHECK(idx, hipGetLastError());
    HIPCHECK(idx, hipMemcpyAsync(m->cand_ctl_host.p, ctl_f, 2 * kPQ * sizeof(int), hipMemcpyDeviceToHost, s));
    if (!c.out_dev) {  // (hd also staged `te`: its H2D copy precedes these copies in stream order)
        HIPCHECK(idx, hipMemcpyAsync(c.hd, m->out_d.p, (size_t)p.n * k * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHECK(idx, hipMemcpyAsync(c.hr, m->out_r.p, (size_t)p.n * k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(idx, hipStreamSynchronize(s));
    if (ms_prof(c)) ms_read_profile(idx, true);
    for (int r = 0; r < p.n; ++r) {
        if (m->cand_ctl_host.p[2 * r + 1] != 0) continue;  // list overflow: exact full scan (the caller's)
        handled[r] = true;
        (c.list ? idx->s_mss_screened : idx->s_ms_screened)++;
        if (!c.list) idx->s_ms_candidates += m->cand_ctl_host.p[2 * r];
        float* od = c.out_dist + (int64_t)p.b[r] * k;
        int64_t* orow = c.out_rows + (int64_t)p.b[r] * k;
        if (c.out_dev) {
            HIPCHECK(idx, hipMemcpyAsync(od, m->out_d.p + (size_t)r * k, k * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIPCHECK(idx, hipMemcpyAsync(orow, m->out_r.p + (size_t)r * k, k * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        } else {
            memcpy(od, &c.hd[(size_t)r * k], k * sizeof(float));
            memcpy(orow, &c.hr[(size_t)r * k], k * sizeof(int64_t));
        }
    }
    return MI355DR_OK;
}

// ---- k above the fast path's, query r of the pass: screen top-k -> candidates -> exact kernel on the candidates -> exact top-k
int ms_slow_query(const MsSearch& c, const MsPass& p, int r) {
    mi355dr_index* idx = c.idx;
    MultiVecStore* m = c.m;
    hipStream_t s = c.s;
    int cur = 0;
    const float* dist16 = m->dist16.p + (int64_t)r * m->n_docs;
    CHECK(ms_topk(c, dist16, m->n_docs, nullptr, nullptr, &cur));
    HIPCHECK(idx, hipMemsetAsync(m->cand_ctl.p, 0, 2 * sizeof(int), s));
    float te = (float)p.two_e[r];
    if ((double)te < p.two_e[r]) te = std::nextafter(te, INFINITY);
    hipLaunchKernelGGL(k_ms_candidates, dim3((unsigned)((m->n_docs + 255) / 256)), dim3(256), 0, s, dist16, c.has_vec,
                       m->n_docs, m->pk[cur].p, c.k, te, m->cand_list.p, kMsCandCap, m->cand_ctl.p);
    HIPCHECK(idx, hipGetLastError());
    MsArgs a = c.a0;
    a.qtok = m->qtok.p + (int64_t)p.col0[r] * m->dpad;
    a.dist = m->cand_dist.p;
    a.doc_list = m->cand_list.p;
    a.n_items = c.n_cand_max;
    a.n_items_dev = m->cand_ctl.p;
    a.nq_launch = 1;
    a.q_col0[0] = 0;
    a.q_len[0] = p.len[r];
    hipLaunchKernelGGL(k_maxsim, dim3((unsigned)std::min<int64_t>((c.n_cand_max + 3) / 4, kMsListGrid)),
                       dim3(kMsThreads), c.lds, s, a);
    HIPCHECK(idx, hipGetLastError());
    CHECK(ms_topk(c, m->cand_dist.p, c.n_cand_max, m->cand_list.p, m->cand_ctl.p, &cur));
    CHECK(ms_emit_result(c, cur, p.b[r]));
    HIPCHECK(idx, hipMemcpyAsync(m->cand_ctl_host.p, m->cand_ctl.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    if (m->cand_ctl_host.p[1] == 0) {
        (c.list ? idx->s_mss_screened : idx->s_ms_screened)++;
        if (!c.list) idx->s_ms_candidates += m->cand_ctl_host.p[0];
    } else {
        (c.list ? idx->s_mss_fallbacks : idx->s_ms_fallbacks)++;  // more candidates than the list holds: this query takes the exact full scan
        CHECK(ms_full_scan_query(c, p.col0[r], p.len[r], p.b[r]));
    }
    return MI355DR_OK;
}

// qtok: HOST [sum_nq, dim]; outputs on the host (out_dev = false) or in device memory of the index's GPU (out_dev = true:
// written by kernels / device copies on the index's stream, complete on return).
// sub (mi355dr_search_maxsim_subset; nullptr: every document): the listed documents with vectors -- local, ascending, unique --
// on the HOST; the store's sub_list / sub_memb buffers already have room for them.
int search_maxsim_impl(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k, float* out_dist,
                       int64_t* out_rows, bool out_dev, const std::vector<int32_t>* sub = nullptr) {
    if (k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "k exceeds 1024");
    if (out_dev) {
        if (B > 0) {
            HIPCHECK(idx, hipSetDevice(idx->device));
            const int64_t n = (int64_t)B * k;
            hipLaunchKernelGGL(k_ms_fill_empty, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->stream, out_dist, out_rows, n);
            HIPCHECK(idx, hipGetLastError());
            HIPCHECK(idx, hipStreamSynchronize(idx->stream));
        }
    } else {
        for (int64_t i = 0; i < (int64_t)B * k; ++i) {
            out_dist[i] = NAN;
            out_rows[i] = -1;
        }
    }
    MultiVecStore* m = idx->mv;
    if (B == 0 || !m || m->n_docs == 0 || (sub && sub->empty())) return MI355DR_OK;
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] - q_offsets[b] < 0) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    HIPCHECK(idx, hipSetDevice(idx->device));
    MsSearch c{idx, m, idx->stream, qtok, q_offsets, B, k, out_dist, out_rows, out_dev};
    if (sub) {
        c.list = m->sub_list.p;
        c.n_list = (int64_t)sub->size();
        c.list_screen = idx->maxsim_subset_screen > 0 || (idx->maxsim_subset_screen < 0 && c.n_list >= idx->maxsim_subset_screen_min);
    }
    CHECK(ms_search_prepare(c));
    if (sub) {
        HIPCHECK(idx, hipMemcpyAsync(m->sub_list.p, sub->data(), sub->size() * sizeof(int32_t), hipMemcpyHostToDevice, c.s));
        if (c.list_screen && m->finite && c.lds16 <= 160 * 1024) {  // (what ms_plan_pass asks of a pass that screens)
            hipLaunchKernelGGL(k_ms_membership, dim3((unsigned)((m->n_docs + 256) / 256)), dim3(256), 0, c.s, m->sub_list.p, c.n_list,
                               m->n_docs, m->sub_memb.p);
            HIPCHECK(idx, hipGetLastError());
        }
    }
    int b = 0;
    while (b < B) {
        HIPCHECK(idx, hipStreamSynchronize(c.s));  // the staging buffers are free again
        if (q_offsets[b + 1] - q_offsets[b] > c.cols) {
            CHECK(ms_run_long_query(c, b));
            ++b;
            continue;
        }
        const MsPass p = ms_plan_pass(c, b);
        b = p.b_end;
        if (p.n == 0) continue;
        const size_t img_cols = std::min<size_t>(kMsImgCols, (size_t)((p.total_col + 31) / 32 * 32 + 32));
        HIPCHECK(idx, hipMemcpyAsync(m->qtok.p, c.qimg, img_cols * m->dpad * sizeof(float), hipMemcpyHostToDevice, c.s));
        if (!p.screen) {
            CHECK(ms_run_exact_group(c, p));
            continue;
        }
        CHECK(ms_launch_screen(c, p));
        bool handled[kPQ] = {};
        if (k <= kMsFastK) {
            CHECK(ms_fast_path(c, p, handled));
        } else if (ms_prof(c)) {  // (the screen launch of a slow-path pass is timed too)
            HIPCHECK(idx, hipStreamSynchronize(c.s));
            ms_read_profile(idx, false);
        }
        for (int r = 0; r < p.n; ++r) {
            if (handled[r]) continue;
            if (k <= kMsFastK) {  // the fast path gave this query up (candidate list overflow): exact full scan
                (c.list ? idx->s_mss_fallbacks : idx->s_ms_fallbacks)++;
                CHECK(ms_full_scan_query(c, p.col0[r], p.len[r], p.b[r]));
            } else {
                CHECK(ms_slow_query(c, p, r));
            }
        }
    }
    HIPCHECK(idx, hipStreamSynchronize(c.s));  // (device outputs: the last copies)
    return MI355DR_OK;
}

// The query vectors of a _device entry point come down once: the query side of a pass is tiny (8 queries x 32 vectors x 128 dims
// = 128 KiB) and its bound is evaluated in double on the host; the k results of every query never leave HBM.  `stream` (may be
// null) produced qtok_dev.  qh / off: the vectors and their offsets from 0.
int ms_fetch_queries(mi355dr_index* idx, const float* qtok_dev, const int32_t* q_offsets, int B, void* stream, std::vector<float>& qh,
                     std::vector<int32_t>& off) {
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] < q_offsets[b]) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    const int64_t n_tok = q_offsets[B] - q_offsets[0];
    if (n_tok > 0 && !qtok_dev) return fail(idx, MI355DR_E_INVALID, "null query vectors");
    HIPCHECK(idx, hipSetDevice(idx->device));
    if (stream) HIPCHECK(idx, hipStreamSynchronize((hipStream_t)stream));
    qh.resize((size_t)std::max<int64_t>(n_tok, 1) * idx->dim);
    if (n_tok > 0)
        HIPCHECK(idx, hipMemcpy(qh.data(), qtok_dev + (int64_t)q_offsets[0] * idx->dim, (size_t)n_tok * idx->dim * sizeof(float),
                                hipMemcpyDeviceToHost));
    off.resize((size_t)B + 1);
    for (int b = 0; b <= B; ++b) off[b] = q_offsets[b] - q_offsets[0];
    return MI355DR_OK;
}

// ---- MaxSim top-k within a listed subset of documents: search_maxsim_impl over the list.
// out_dev: qtok and the outputs are device memory (the rule of mi355dr_search_maxsim_device); doc_ids and q_offsets are host.
int search_maxsim_subset_impl(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k, const int64_t* doc_ids,
                              int64_t m_ids, float* out_dist, int64_t* out_rows, bool out_dev, void* stream) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "search_maxsim_subset", /*ask_parent=*/true);
    if (B < 0 || k <= 0 || !q_offsets || m_ids < 0 || (m_ids > 0 && !doc_ids) || (B > 0 && (!out_dist || !out_rows)))
        return fail(idx, MI355DR_E_INVALID, "bad search_maxsim_subset arguments");
    if (k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "k exceeds 1024");
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] < q_offsets[b]) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    MultiVecStore* m = idx->mv;
    // the caller's global ids -> the listed documents with vectors: local, ascending, unique (subset_ids.h)
    std::vector<int32_t> list;
    if (B > 0 && m && m->n_docs > 0 && m_ids > 0) {
        try {
            subset_prepare_ids(doc_ids, m_ids, idx->row_offset, m->n_docs, list);
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "search_maxsim_subset: out of host memory for the document list");
        }
        const std::vector<int64_t>& off = m->blk_off_host;
        list.erase(std::remove_if(list.begin(), list.end(), [&](int32_t d) { return off[(size_t)d + 1] <= off[(size_t)d]; }), list.end());
    }
    if (!list.empty()) {  // room for the list and the table before anything is launched
        HIPCHECK(idx, hipSetDevice(idx->device));
        HIPCHECK(idx, m->sub_list.grow(list.size() * sizeof(int32_t)));
        HIPCHECK(idx, m->sub_memb.grow((size_t)(m->cap_docs + 1) * sizeof(int64_t)));
    }
    std::vector<float> qh;
    std::vector<int32_t> off;
    if (out_dev && B > 0) {
        CHECK(ms_fetch_queries(idx, qtok, q_offsets, B, stream, qh, off));
        qtok = qh.data();
        q_offsets = off.data();
    }
    CHECK(search_maxsim_impl(idx, qtok, q_offsets, B, k, out_dist, out_rows, out_dev, &list));
    idx->s_mss_searches++;
    idx->s_mss_docs += (int64_t)list.size();
    return MI355DR_OK;
}

int maxsim_subset_impl(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids,
                       int m_ids, int clamp0, float* out_dist) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "maxsim_subset", /*ask_parent=*/true);
    if (B < 0 || m_ids < 0 || !q_offsets || (B > 0 && m_ids > 0 && (!doc_ids || !out_dist)))
        return fail(idx, MI355DR_E_INVALID, "bad maxsim_subset arguments");
    for (int64_t i = 0; i < (int64_t)B * m_ids; ++i) out_dist[i] = NAN;
    MultiVecStore* m = idx->mv;
    if (B == 0 || m_ids == 0 || !m || m->n_docs == 0) return MI355DR_OK;
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] - q_offsets[b] < 0) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    HIPCHECK(idx, hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    const int dp = m->dpad, d = idx->dim;
    const int cols = ms_cols_for(dp);  // query vectors per launch; a longer query is scored in tiles (MsArgs::dist_in)
    if (cols < 32) return fail(idx, MI355DR_E_UNSUPPORTED, "dim too large for the MaxSim kernel's LDS budget (dim <= 1272)");
    const size_t lds = (size_t)cols * (dp + 4) * sizeof(float);
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_maxsim, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds + kMsRedBytes)));
    std::vector<int32_t> list((size_t)B * m_ids);
    for (int64_t i = 0; i < (int64_t)B * m_ids; ++i) {
        const int64_t v = doc_ids[i] - idx->row_offset;  // ids are global rows, like the search results
        list[i] = (v >= 0 && v < m->n_docs) ? (int32_t)v : -1;
    }
    // per call scratch (candidate lists are small: a few hundred docs per query)
    DevBuf<int32_t> list_dev;
    DevBuf<float> dist_dev, q_dev;
    HIPCHECK(idx, list_dev.grow(list.size() * sizeof(int32_t)));
    HIPCHECK(idx, dist_dev.grow(list.size() * sizeof(float)));
    HIPCHECK(idx, q_dev.grow((size_t)cols * dp * sizeof(float)));
    HIPCHECK(idx, hipMemcpyAsync(list_dev.p, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    std::vector<float> qimg((size_t)cols * dp);
    for (int b = 0; b < B; ++b) {
        const int nq = q_offsets[b + 1] - q_offsets[b];
        if (nq == 0) continue;  // reference heaven.py:251-252: no query vectors -> every score 0 (host side)
        for (int t0 = 0; t0 < nq; t0 += cols) {  // tiles of the query's vectors: each launch continues the per-doc sums
            const int tl = std::min(cols, nq - t0);
            std::fill(qimg.begin(), qimg.end(), 0.0f);
            for (int j = 0; j < tl; ++j)
                multivec_pack_query_row(qtok + (int64_t)(q_offsets[b] + t0 + j) * d, d, dp, &qimg[(size_t)j * dp]);
            // the staging buffer is reused: the previous launch must have consumed it (stream order + pageable copy)
            HIPCHECK(idx, hipMemcpyAsync(q_dev.p, qimg.data(), qimg.size() * sizeof(float), hipMemcpyHostToDevice, s));
            HIPCHECK(idx, hipStreamSynchronize(s));
            MsArgs a{};
            a.tok = m->tok.p;
            a.blk_off = m->blk_off.p;
            a.qtok = q_dev.p;
            a.dist = dist_dev.p + (int64_t)b * m_ids;
            a.dist_in = t0 > 0 ? a.dist : nullptr;
            a.doc_list = list_dev.p + (int64_t)b * m_ids;
            a.n_items = m_ids;
            a.n_docs = m->n_docs;
            a.dpad = dp;
            a.nq_launch = 1;
            a.q_col0[0] = 0;
            a.q_len[0] = tl;
            a.clamp0 = clamp0;
            hipLaunchKernelGGL(k_maxsim, dim3((unsigned)std::min<int64_t>((m_ids + 3) / 4, kMsListGrid)), dim3(kMsThreads),
                               lds, s, a);
            HIPCHECK(idx, hipGetLastError());
        }
        HIPCHECK(idx, hipMemcpyAsync(out_dist + (int64_t)b * m_ids, dist_dev.p + (int64_t)b * m_ids, m_ids * sizeof(float),
                                     hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(idx, hipStreamSynchronize(s));
    return MI355DR_OK;
}

// ---- MaxSim explained: the terms of the sum (k_maxsim_align.h) ----

// token vectors of local document v; -1: not a document of this store
inline int32_t ms_token_count(const MultiVecStore* m, int64_t v) {
    return (m && v >= 0 && v < m->n_docs) ? m->tok_cnt_host[(size_t)v] : -1;
}

int multivec_token_counts_impl(mi355dr_index* idx, const int64_t* doc_ids, int64_t n, int32_t* out_counts) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "multivec_token_counts", /*ask_parent=*/true);
    if (n < 0 || (n > 0 && (!doc_ids || !out_counts))) return fail(idx, MI355DR_E_INVALID, "bad multivec_token_counts arguments");
    for (int64_t j = 0; j < n; ++j) out_counts[j] = ms_token_count(idx->mv, doc_ids[j] - idx->row_offset);
    return MI355DR_OK;
}

// what both calls share on the device: every query vector packed in the store's column order, and the tile table
struct MsAlignScratch {
    DevBuf<float> q_dev;
    DevBuf<MsAlignTile> tiles_dev;
    std::vector<float> qimg;
    std::vector<MsAlignTile> tiles;
};

// dim bound and the kernels' dynamic LDS; *cols = query vectors per tile
int ms_align_prepare(mi355dr_index* idx, const MultiVecStore* m, int* cols, size_t* lds) {
    *cols = ms_cols_for(m->dpad);
    if (*cols < 32) return fail(idx, MI355DR_E_UNSUPPORTED, "dim too large for the MaxSim kernel's LDS budget (dim <= 1272)");
    *lds = (size_t)*cols * (m->dpad + 4) * sizeof(float);
    HIPCHECK(idx, hipSetDevice(idx->device));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_maxsim_align, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
    HIPCHECK(idx, hipFuncSetAttribute((const void*)k_maxsim_map, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
    return MI355DR_OK;
}

// allocate, then upload (nothing is launched before every buffer of the call is there: the caller grows its own first)
int ms_align_upload(mi355dr_index* idx, MsAlignScratch& w, hipStream_t s) {
    HIPCHECK(idx, hipMemcpyAsync(w.q_dev.p, w.qimg.data(), w.qimg.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHECK(idx, hipMemcpyAsync(w.tiles_dev.p, w.tiles.data(), w.tiles.size() * sizeof(MsAlignTile), hipMemcpyHostToDevice, s));
    return MI355DR_OK;
}

void ms_align_pack_queries(const MultiVecStore* m, int d, const float* qtok, const int32_t* q_offsets, int B, std::vector<float>& qimg) {
    const int64_t V = q_offsets[B] - q_offsets[0];
    qimg.resize((size_t)V * m->dpad);
    for (int64_t g = 0; g < V; ++g)
        multivec_pack_query_row(qtok + (q_offsets[0] + g) * d, d, m->dpad, &qimg[(size_t)g * m->dpad]);
}

int maxsim_align_impl(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids, int m_ids,
                      int flags, float* out_val, int32_t* out_tok, float* out_dist) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "maxsim_align", /*ask_parent=*/true);
    if (flags & ~MI355DR_MAXSIM_CLAMP0) return fail(idx, MI355DR_E_INVALID, "unknown maxsim flag");
    if (B < 0 || m_ids < 0 || (B > 0 && !q_offsets)) return fail(idx, MI355DR_E_INVALID, "bad maxsim_align arguments");
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] < q_offsets[b]) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    const int64_t V = B > 0 ? (int64_t)q_offsets[B] - q_offsets[0] : 0;
    const int64_t mm = m_ids, n_val = V * mm, n_dist = (int64_t)B * mm;
    if ((n_val > 0 && (!qtok || !out_val || !out_tok)) || (n_dist > 0 && !doc_ids))
        return fail(idx, MI355DR_E_INVALID, "maxsim_align: null pointer");
    for (int64_t i = 0; i < n_val; ++i) {
        out_val[i] = NAN;
        out_tok[i] = -1;
    }
    if (out_dist)
        for (int64_t i = 0; i < n_dist; ++i) out_dist[i] = NAN;
    idx->s_msa_calls++;
    MultiVecStore* m = idx->mv;
    if (n_val == 0 || !m || m->n_docs == 0) return MI355DR_OK;
    int cols = 0;
    size_t lds = 0;
    CHECK(ms_align_prepare(idx, m, &cols, &lds));
    hipStream_t s = idx->stream;
    MsAlignScratch w;
    std::vector<int32_t> list;
    int64_t pairs = 0;
    try {
        list.resize((size_t)n_dist);
        for (int b = 0; b < B; ++b) {
            const int nq = q_offsets[b + 1] - q_offsets[b];
            for (int64_t p = 0; p < mm; ++p) {
                const int64_t v = doc_ids[b * mm + p] - idx->row_offset;  // ids are global rows, like the search results
                const bool mine = v >= 0 && v < m->n_docs;
                list[(size_t)(b * mm + p)] = mine ? (int32_t)v : -1;
                if (mine && nq > 0 && m->tok_cnt_host[(size_t)v] > 0) ++pairs;
            }
            for (int t0 = 0; t0 < nq; t0 += cols)
                w.tiles.push_back(MsAlignTile{q_offsets[b] - q_offsets[0] + t0, std::min(cols, nq - t0), b, 0, 0, 0, 0});
        }
        ms_align_pack_queries(m, idx->dim, qtok, q_offsets, B, w.qimg);
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "maxsim_align: out of host memory");
    }
    DevBuf<int32_t> list_dev, tok_dev, qoff_dev;
    DevBuf<float> val_dev, dist_dev;
    HIPCHECK(idx, w.q_dev.grow(w.qimg.size() * sizeof(float)));
    HIPCHECK(idx, w.tiles_dev.grow(w.tiles.size() * sizeof(MsAlignTile)));
    HIPCHECK(idx, list_dev.grow(list.size() * sizeof(int32_t)));
    HIPCHECK(idx, val_dev.grow((size_t)n_val * sizeof(float)));
    HIPCHECK(idx, tok_dev.grow((size_t)n_val * sizeof(int32_t)));
    if (out_dist) {
        HIPCHECK(idx, dist_dev.grow((size_t)n_dist * sizeof(float)));
        HIPCHECK(idx, qoff_dev.grow((size_t)(B + 1) * sizeof(int32_t)));
    }
    CHECK(ms_align_upload(idx, w, s));
    HIPCHECK(idx, hipMemcpyAsync(list_dev.p, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    std::vector<int32_t> qoff((size_t)B + 1);
    for (int b = 0; b <= B; ++b) qoff[(size_t)b] = q_offsets[b] - q_offsets[0];
    if (out_dist) HIPCHECK(idx, hipMemcpyAsync(qoff_dev.p, qoff.data(), qoff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    MsAlignArgs a{};
    a.tok = m->tok.p;
    a.blk_off = m->blk_off.p;
    a.qtok = w.q_dev.p;
    a.doc_list = list_dev.p;
    a.out_val = val_dev.p;
    a.out_tok = tok_dev.p;
    a.m = mm;
    a.n_docs = m->n_docs;
    a.dpad = m->dpad;
    a.clamp0 = (flags & MI355DR_MAXSIM_CLAMP0) ? 1 : 0;
    const unsigned gx = (unsigned)std::min<int64_t>((mm + 3) / 4, kMsListGrid);
    for (size_t t0 = 0; t0 < w.tiles.size(); t0 += 65535) {  // one workgroup row per tile; every vector owns its output row
        a.tiles = w.tiles_dev.p + t0;
        hipLaunchKernelGGL(k_maxsim_align, dim3(gx, (unsigned)std::min<size_t>(65535, w.tiles.size() - t0)), dim3(kMsThreads), lds, s, a);
        HIPCHECK(idx, hipGetLastError());
    }
    if (out_dist) {
        hipLaunchKernelGGL(k_maxsim_align_dist, dim3((unsigned)((n_dist + 255) / 256)), dim3(256), 0, s, val_dev.p, qoff_dev.p, B, mm,
                           dist_dev.p);
        HIPCHECK(idx, hipGetLastError());
        HIPCHECK(idx, hipMemcpyAsync(out_dist, dist_dev.p, (size_t)n_dist * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(idx, hipMemcpyAsync(out_val, val_dev.p, (size_t)n_val * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipMemcpyAsync(out_tok, tok_dev.p, (size_t)n_val * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    idx->s_msa_pairs += pairs;
    return MI355DR_OK;
}

int maxsim_map_impl(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int32_t* pair_query,
                    const int64_t* pair_doc, int64_t P, const int64_t* out_offsets, float* out) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "maxsim_map", /*ask_parent=*/true);
    if (B < 0 || P < 0 || (B > 0 && !q_offsets) || (P > 0 && (!pair_query || !pair_doc || !out_offsets)))
        return fail(idx, MI355DR_E_INVALID, "bad maxsim_map arguments");
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] < q_offsets[b]) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    MultiVecStore* m = idx->mv;
    int cols = 32;
    size_t lds = 0;
    if (P > 0 && m && m->n_docs > 0) CHECK(ms_align_prepare(idx, m, &cols, &lds));
    MsAlignScratch w;
    try {
        for (int64_t p = 0; p < P; ++p) {
            if (pair_query[p] < 0 || pair_query[p] >= B) return fail(idx, MI355DR_E_INVALID, "maxsim_map: pair_query out of range");
            const int b = pair_query[p];
            const int64_t v = pair_doc[p] - idx->row_offset;
            const int nq = q_offsets[b + 1] - q_offsets[b];
            const int64_t T = std::max<int64_t>(ms_token_count(m, v), 0);
            if (out_offsets[p + 1] - out_offsets[p] != nq * T)
                return fail(idx, MI355DR_E_INVALID, "maxsim_map: a slot must hold exactly nq * T floats (mi355dr_multivec_token_counts)");
            if (nq * T == 0) continue;
            for (int t0 = 0; t0 < nq; t0 += cols)
                w.tiles.push_back(MsAlignTile{q_offsets[b] - q_offsets[0] + t0, std::min(cols, nq - t0), b, (int)v, (int)T, 0,
                                              out_offsets[p] - out_offsets[0] + t0 * T});
        }
        const int64_t total = P > 0 ? out_offsets[P] - out_offsets[0] : 0;
        if (total > 0 && (!out || !qtok)) return fail(idx, MI355DR_E_INVALID, "maxsim_map: null pointer");
        idx->s_msm_calls++;
        if (total == 0) return MI355DR_OK;
        ms_align_pack_queries(m, idx->dim, qtok, q_offsets, B, w.qimg);
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "maxsim_map: out of host memory");
    }
    const int64_t total = out_offsets[P] - out_offsets[0];
    hipStream_t s = idx->stream;
    DevBuf<float> out_dev;
    HIPCHECK(idx, w.q_dev.grow(w.qimg.size() * sizeof(float)));
    HIPCHECK(idx, w.tiles_dev.grow(w.tiles.size() * sizeof(MsAlignTile)));
    HIPCHECK(idx, out_dev.grow((size_t)total * sizeof(float)));
    CHECK(ms_align_upload(idx, w, s));
    MsAlignArgs a{};
    a.tok = m->tok.p;
    a.blk_off = m->blk_off.p;
    a.qtok = w.q_dev.p;
    a.tiles = w.tiles_dev.p;
    a.out_val = out_dev.p;
    a.n_docs = m->n_docs;
    a.dpad = m->dpad;
    hipLaunchKernelGGL(k_maxsim_map, dim3((unsigned)w.tiles.size()), dim3(kMsThreads), lds, s, a);
    HIPCHECK(idx, hipGetLastError());
    HIPCHECK(idx, hipMemcpyAsync(out + out_offsets[0], out_dev.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    idx->s_msm_values += total;
    return MI355DR_OK;
}

// ---- test hook: one pass of the search above, observed (mi355dr_debug_maxsim_pass, include/mi355dr.h) ----
// what a pass counts and the one option the hook switches off for its own pass, put back on every way out
struct MsDebugKeep {
    mi355dr_index* idx;
    int profile;
    int64_t screened, candidates, fallbacks, cols, packed, ss, se, sf;
    explicit MsDebugKeep(mi355dr_index* i)
        : idx(i), profile(i->profile), screened(i->s_ms_screened), candidates(i->s_ms_candidates), fallbacks(i->s_ms_fallbacks),
          cols(i->s_ms_screen_cols), packed(i->s_ms_packed_launches), ss(i->s_mss_screened), se(i->s_mss_exact), sf(i->s_mss_fallbacks) {
        idx->profile = 0;  // (no events, no timing stats)
    }
    ~MsDebugKeep() {
        idx->profile = profile;
        idx->s_ms_screened = screened;
        idx->s_ms_candidates = candidates;
        idx->s_ms_fallbacks = fallbacks;
        idx->s_ms_screen_cols = cols;
        idx->s_ms_packed_launches = packed;
        idx->s_mss_screened = ss;
        idx->s_mss_exact = se;
        idx->s_mss_fallbacks = sf;
    }
};

int debug_maxsim_pass_impl(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k, const int64_t* doc_ids,
                           int64_t m_ids, int list_cap, int* out_live, float* out_screen, float* out_two_e, int32_t* out_lists,
                           int* out_ctl, float* out_wide_sd, int* out_form, int* out_info) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return fail(idx, MI355DR_E_INVALID, "debug_maxsim_pass: not on a view");
    if (B <= 0 || B > kPQ || k <= 0 || k > kKMax || !qtok || !q_offsets || m_ids < 0 || list_cap < 1 || !out_live || !out_screen ||
        !out_two_e || !out_lists || !out_ctl || !out_wide_sd || !out_form || !out_info)
        return fail(idx, MI355DR_E_INVALID, "bad debug_maxsim_pass arguments");
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] < q_offsets[b]) return fail(idx, MI355DR_E_INVALID, "q_offsets must be non-decreasing");
    MultiVecStore* m = idx->mv;
    if (!m || m->n_docs == 0) return fail(idx, MI355DR_E_INVALID, "debug_maxsim_pass: the index has no multi-vector store");
    HIPCHECK(idx, hipSetDevice(idx->device));
    // a document list: what search_maxsim_subset_impl and search_maxsim_impl do with it before the first pass
    std::vector<int32_t> list;
    if (doc_ids) {
        try {
            subset_prepare_ids(doc_ids, m_ids, idx->row_offset, m->n_docs, list);
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "debug_maxsim_pass: out of host memory for the document list");
        }
        const std::vector<int64_t>& off = m->blk_off_host;
        list.erase(std::remove_if(list.begin(), list.end(), [&](int32_t d) { return off[(size_t)d + 1] <= off[(size_t)d]; }), list.end());
        if (list.empty()) return fail(idx, MI355DR_E_INVALID, "debug_maxsim_pass: no listed document has vectors");
        HIPCHECK(idx, m->sub_list.grow(list.size() * sizeof(int32_t)));
        HIPCHECK(idx, m->sub_memb.grow((size_t)(m->cap_docs + 1) * sizeof(int64_t)));
    }
    MsDebugKeep keep(idx);
    std::vector<float> res_d((size_t)B * k);  // the fast path's results: not reported
    std::vector<int64_t> res_r((size_t)B * k);
    MsSearch c{idx, m, idx->stream, qtok, q_offsets, B, k, res_d.data(), res_r.data(), false};
    if (doc_ids) {
        c.list = m->sub_list.p;
        c.n_list = (int64_t)list.size();
        c.list_screen = idx->maxsim_subset_screen > 0 || (idx->maxsim_subset_screen < 0 && c.n_list >= idx->maxsim_subset_screen_min);
    }
    CHECK(ms_search_prepare(c));
    for (int b = 0; b < B; ++b)
        if (q_offsets[b + 1] - q_offsets[b] > c.cols)
            return fail(idx, MI355DR_E_INVALID, "debug_maxsim_pass: a query has more vectors than one launch stages");
    if (doc_ids) {
        HIPCHECK(idx, hipMemcpyAsync(m->sub_list.p, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.s));
        if (c.list_screen && m->finite && c.lds16 <= 160 * 1024) {
            hipLaunchKernelGGL(k_ms_membership, dim3((unsigned)((m->n_docs + 256) / 256)), dim3(256), 0, c.s, m->sub_list.p, c.n_list,
                               m->n_docs, m->sub_memb.p);
            HIPCHECK(idx, hipGetLastError());
        }
    }
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    const MsPass p = ms_plan_pass(c, 0);
    if (p.b_end < B) return fail(idx, MI355DR_E_INVALID, "debug_maxsim_pass: the queries do not fit one pass");
    for (int b = 0; b < B; ++b) out_live[b] = -1;
    for (int r = 0; r < p.n; ++r) out_live[p.b[r]] = r;
    idx->last_screen_form = {};
    out_info[0] = p.n;
    out_info[1] = kMsCandCap;
    out_info[2] = 0;
    out_info[3] = kMsTightenMax;
    for (int i = 0; i < 8; ++i) out_form[i] = 0;
    for (int r = 0; r < p.n; ++r) {  // (the rounding of ms_fast_path / ms_slow_query; the fast path's device copy replaces it below)
        out_two_e[r] = (float)p.two_e[r];
        if ((double)out_two_e[r] < p.two_e[r]) out_two_e[r] = std::nextafter(out_two_e[r], INFINITY);
    }
    if (p.n == 0 || !p.screen) return MI355DR_OK;
    const size_t img_cols = std::min<size_t>(kMsImgCols, (size_t)((p.total_col + 31) / 32 * 32 + 32));
    HIPCHECK(idx, hipMemcpyAsync(m->qtok.p, c.qimg, img_cols * m->dpad * sizeof(float), hipMemcpyHostToDevice, c.s));
    const size_t screen_bytes = (size_t)p.n * m->n_docs * sizeof(float);
    HIPCHECK(idx, hipMemsetAsync(m->dist16.p, 0xFF, screen_bytes, c.s));
    CHECK(ms_launch_screen(c, p));
    HIPCHECK(idx, hipMemcpyAsync(out_screen, m->dist16.p, screen_bytes, hipMemcpyDeviceToHost, c.s));
    HIPCHECK(idx, hipStreamSynchronize(c.s));
    const auto& f = idx->last_screen_form;
    const int form[8] = {f.family, f.ncb, f.waves, f.bps, f.pipe, f.now, f.grid, 0};
    memcpy(out_form, form, sizeof(form));
    if (k > kMsFastK) return MI355DR_OK;
    bool handled[kPQ] = {};
    CHECK(ms_fast_path(c, p, handled));
    std::vector<int32_t> lists((size_t)3 * kPQ * kMsCandCap);
    std::vector<float> sd((size_t)kPQ * kMsCandCap);
    int ctl[3 * 2 * kPQ];
    HIPCHECK(idx, hipMemcpy(lists.data(), m->cand_list.p, lists.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(idx, hipMemcpy(sd.data(), m->cand_sd.p, sd.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(idx, hipMemcpy(ctl, m->cand_ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
    HIPCHECK(idx, hipMemcpy(out_two_e, m->two_e_dev.p, p.n * sizeof(float), hipMemcpyDeviceToHost));
    const bool tighten = idx->maxsim_tighten != 0;
    for (int sec = 0; sec < 3; ++sec) {
        const int src = sec == 2 && !tighten ? 0 : sec;  // (ms_fast_path: without the tightening the final list is the wide list)
        for (int r = 0; r < p.n; ++r) {
            const int cnt = ctl[(src * kPQ + r) * 2];
            out_ctl[(sec * B + r) * 2] = cnt;
            out_ctl[(sec * B + r) * 2 + 1] = ctl[(src * kPQ + r) * 2 + 1];
            const size_t n = (size_t)std::min({cnt, kMsCandCap, list_cap});
            memcpy(out_lists + ((size_t)sec * B + r) * list_cap, &lists[((size_t)src * kPQ + r) * kMsCandCap], n * sizeof(int32_t));
            if (sec == 0 && tighten) memcpy(out_wide_sd + (size_t)r * list_cap, &sd[(size_t)r * kMsCandCap], n * sizeof(float));
        }
    }
    out_info[2] = 1;
    return MI355DR_OK;
}

}  // namespace

namespace mi355 {
int multivec_reserve(mi355dr_index* idx, int64_t n_blocks, int64_t n_docs) {
    std::lock_guard<std::mutex> g(idx->mu);
    HIPCHECK(idx, hipSetDevice(idx->device));
    return ms_reserve(idx, ms_store(idx), n_blocks, n_docs);
}
}  // namespace mi355

extern "C" {

int mi355dr_add_multivec(mi355dr_index* idx, const float* vecs, const int64_t* offsets, int64_t n_docs) {
    return ms_add(idx, vecs, offsets, n_docs, false);
}

int mi355dr_add_multivec_device(mi355dr_index* idx, const float* vecs_dev, const int64_t* offsets, int64_t n_docs) {
    return ms_add(idx, vecs_dev, offsets, n_docs, true);
}

int mi355dr_set_multivec(mi355dr_index* idx, const int64_t* doc_ids, const float* vecs, const int64_t* offsets, int64_t n) {
    return ms_set(idx, doc_ids, vecs, offsets, n, false);
}

int mi355dr_set_multivec_device(mi355dr_index* idx, const int64_t* doc_ids, const float* vecs_dev, const int64_t* offsets, int64_t n) {
    return ms_set(idx, doc_ids, vecs_dev, offsets, n, true);
}

int64_t mi355dr_size_multivec(const mi355dr_index* idx) { return idx && idx->mv ? idx->mv->n_docs : 0; }

int64_t mi355dr_live_multivec(const mi355dr_index* idx) { return idx && idx->mv ? idx->mv->n_live : 0; }

int mi355dr_search_maxsim(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k,
                          float* out_dist, int64_t* out_rows) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B < 0 || k <= 0 || !q_offsets || (B > 0 && (!out_dist || !out_rows)))
        return fail(idx, MI355DR_E_INVALID, "bad maxsim arguments");
    return search_maxsim_impl(idx, qtok, q_offsets, B, k, out_dist, out_rows, false);
}

int mi355dr_search_maxsim_device(mi355dr_index* idx, const float* qtok_dev, const int32_t* q_offsets, int B, int k,
                                 float* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (B < 0 || k <= 0 || !q_offsets || (B > 0 && (!out_dist_dev || !out_rows_dev)))
        return fail(idx, MI355DR_E_INVALID, "bad maxsim arguments");
    if (B == 0) return MI355DR_OK;
    std::vector<float> qh;
    std::vector<int32_t> off;
    CHECK(ms_fetch_queries(idx, qtok_dev, q_offsets, B, stream, qh, off));
    return search_maxsim_impl(idx, qh.data(), off.data(), B, k, out_dist_dev, out_rows_dev, true);
}

int mi355dr_search_maxsim_subset(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k,
                                 const int64_t* doc_ids, int64_t m, float* out_dist, int64_t* out_rows) {
    return search_maxsim_subset_impl(idx, qtok, q_offsets, B, k, doc_ids, m, out_dist, out_rows, false, nullptr);
}

int mi355dr_search_maxsim_subset_device(mi355dr_index* idx, const float* qtok_dev, const int32_t* q_offsets, int B, int k,
                                        const int64_t* doc_ids, int64_t m, float* out_dist_dev, int64_t* out_rows_dev,
                                        void* stream) {
    return search_maxsim_subset_impl(idx, qtok_dev, q_offsets, B, k, doc_ids, m, out_dist_dev, out_rows_dev, true, stream);
}

int mi355dr_maxsim_subset(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids,
                          int m_ids, float* out_dist) {
    return maxsim_subset_impl(idx, qtok, q_offsets, B, doc_ids, m_ids, 0, out_dist);
}

int mi355dr_maxsim_subset_ex(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids,
                             int m_ids, int flags, float* out_dist) {
    if (flags & ~MI355DR_MAXSIM_CLAMP0) return fail(idx, MI355DR_E_INVALID, "unknown maxsim flag");
    return maxsim_subset_impl(idx, qtok, q_offsets, B, doc_ids, m_ids, (flags & MI355DR_MAXSIM_CLAMP0) ? 1 : 0, out_dist);
}

int mi355dr_multivec_token_counts(mi355dr_index* idx, const int64_t* doc_ids, int64_t n, int32_t* out_counts) {
    return multivec_token_counts_impl(idx, doc_ids, n, out_counts);
}

int mi355dr_maxsim_align(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int64_t* doc_ids, int m,
                         int flags, float* out_val, int32_t* out_tok, float* out_dist) {
    return maxsim_align_impl(idx, qtok, q_offsets, B, doc_ids, m, flags, out_val, out_tok, out_dist);
}

int mi355dr_maxsim_map(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, const int32_t* pair_query,
                       const int64_t* pair_doc, int64_t P, const int64_t* out_offsets, float* out) {
    return maxsim_map_impl(idx, qtok, q_offsets, B, pair_query, pair_doc, P, out_offsets, out);
}

int mi355dr_debug_maxsim_pass(mi355dr_index* idx, const float* qtok, const int32_t* q_offsets, int B, int k, const int64_t* doc_ids,
                              int64_t m, int list_cap, int* out_live, float* out_screen, float* out_two_e, int32_t* out_lists,
                              int* out_ctl, float* out_wide_sd, int* out_form, int* out_info) {
    return debug_maxsim_pass_impl(idx, qtok, q_offsets, B, k, doc_ids, m, list_cap, out_live, out_screen, out_two_e, out_lists, out_ctl,
                                  out_wide_sd, out_form, out_info);
}

}  // extern "C"
