// mi355dr_sparse.hip -- the sparse store of libmi355dr.so: tokenised documents, weighted / BM25 top-k.
// The arithmetic is fixed by include/mi355dr.h ("sparse store"); no bit parity with VectorChord-BM25 is claimed.
//
// Host side: the documents as sorted (term, tf) pairs (6 bytes per posting) with their lengths and df -- what an add appends
// to, what a set / remove replaces a document's slice of, what the BM25 weights are computed from, and what the term-major
// device layout is rebuilt from (counting sort + upload) by the first search after a mutation.  Device side: term_off
// [vocab + 1], postings (doc int32, tf uint16) ascending by document inside a term, document lengths, and the norms of the last
// (k1, b) -- once as the base (the last full build) and, while documents have been replaced, emptied or appended since, a
// `moved` bit per document and an overlay of the same format with those documents' current postings.  A search runs the
// document range in a few launches of growing size (k_sparse.h): the first cannot overflow a candidate list, every later one
// appends only what beats the query's k-th kept entry.  Within a listed subset (the *_subset forms; sparse_subset.h) a long list
// runs the same launches over the tiles that hold a listed document, filtered by a bitmap; a short one, and the score forms,
// look every (query, document) pair up directly (k_sparse_pairs).  Over a row-sharded index (the *_sharded forms; sparse_shard.h,
// k_sparse_shard.h) the same launches run with the statistics of ALL shards -- gathered and summed once
// per call -- and a block's kept lists leave as a packed block for one all-gather and the world * k -> k merge.
#include "index.h"
#include "k_sparse.h"
#include "k_sparse_shard.h"
#include "sparse_shard.h"
#include "sparse_subset.h"
#include "subset_ids.h"

#include <new>

using namespace mi355;

namespace mi355 {

struct SparseStore {
    // host.  Document d is the pairs [doc_at[d], + doc_cnt[d]) of the arena (h_term ascending inside a document, h_tf alongside).
    // The arena is append-only: a set writes the new pairs at its end and leaves the old ones behind; every full layout build
    // squeezes it back to n_post pairs in document order.
    int64_t n_docs = 0, n_live = 0, total_len = 0, n_post = 0;
    int64_t vocab = 0;              // largest term id with df > 0, plus one (df may be longer: zeros behind it)
    std::vector<int32_t> doc_len;   // [n_docs]
    std::vector<int64_t> doc_at;    // [n_docs]
    std::vector<int32_t> doc_cnt;   // [n_docs] distinct terms
    std::vector<int32_t> h_term;
    std::vector<uint16_t> h_tf;
    std::vector<int64_t> df;
    // what the device's base layout holds (the last full build), and what has left it since
    bool has_base = false;
    int64_t base_post = 0;
    int base_vocab = 0;
    std::vector<unsigned> moved;    // [(n_docs + 31) / 32] documents whose content is no longer the base's (appended ones too)
    int64_t moved_post = 0;         // postings the moved documents hold now: the overlay's size once it is built
    int64_t dead_post = 0;          // postings the moved documents have in the base
    // device layout (stale after an add / set / remove until the next search)
    bool stale = false;
    DevBuf<int64_t> term_off, ov_term_off;
    DevBuf<int32_t> post_doc, ov_post_doc, len_dev;
    DevBuf<uint16_t> post_tf, ov_post_tf;
    DevBuf<unsigned> moved_dev;
    int64_t moved_words_dev = 0;
    int ov_vocab = 0;
    bool ov_active = false;         // the layout on the device has moved documents: searches launch k_sparse_score<true>
    int64_t ov_post_dev = 0, dead_post_dev = 0;  // the overlay's postings and the base's dead ones, as built
    DevBuf<double> norm;
    bool norm_valid = false;
    double norm_k1 = 0.0, norm_b = 0.0;
    uint64_t norm_avgdl = 0;        // the bits of the avgdl the norms were computed with: the store's own, or a sharded call's
    // one block's scratch
    DevBuf<int32_t> q_terms, q_off, best_doc, cand_doc;
    DevBuf<double> q_w, out_dist;
    DevBuf<int64_t> out_rows;
    DevBuf<uint64_t> best_key, cand_key;
    DevBuf<unsigned> count;
    DevBuf<int> flags, qlist;
    DevBuf<unsigned long long> scored;
    // a call within a listed subset: the `allowed` bitmap, the launches' tile lists, the local ids and the score forms' distances
    DevBuf<unsigned> sub_bits;
    DevBuf<int32_t> sub_tiles, sub_ids;
    DevBuf<double> pair_dist;
    // a sharded call: this rank's payload of an all-gather, the gathered payloads of all ranks, the folded statistics row
    DevBuf<int64_t> sh_send, sh_recv, sh_fold;
    bool lds_registered = false;
};

void sparse_destroy(mi355dr_index* idx) {
    delete idx->sp;
    idx->sp = nullptr;
}

int64_t sparse_bytes(const mi355dr_index* idx) {
    const SparseStore* s = idx->sp;
    return s ? (int64_t)(s->term_off.bytes + s->post_doc.bytes + s->post_tf.bytes + s->len_dev.bytes + s->norm.bytes +
                         s->ov_term_off.bytes + s->ov_post_doc.bytes + s->ov_post_tf.bytes + s->moved_dev.bytes +
                         s->sub_bits.bytes + s->sub_tiles.bytes + s->sub_ids.bytes + s->pair_dist.bytes + s->sh_send.bytes +
                         s->sh_recv.bytes + s->sh_fold.bytes)
             : 0;
}

int64_t sparse_stat(const mi355dr_index* idx, int which) {
    const SparseStore* s = idx->sp;
    if (!s) return 0;
    switch (which) {
    case kSparseStatDocs: return s->n_live;
    case kSparseStatTotalLen: return s->total_len;
    case kSparseStatPostings: return s->n_post;
    case kSparseStatOverlayPostings: return s->ov_post_dev;
    case kSparseStatDeadPostings: return s->dead_post_dev;
    default: return s->vocab;
    }
}

}  // namespace mi355

namespace {

constexpr int32_t kTermLimit = 1 << 20;
constexpr int kTfMax = 4095;
constexpr int64_t kDocsMax = 0x7FFFFFFEll;

template <class F>
void for_each_moved(const SparseStore* sp, F f) {  // ascending
    for (size_t w = 0; w < sp->moved.size(); ++w)
        for (unsigned bits = sp->moved[w]; bits; bits &= bits - 1) f((int64_t)w * 32 + __builtin_ctz(bits));
}

// a term-major layout (counting sort by term, documents ascending inside a term) in host vectors: of every document, or of
// the moved ones alone
struct HostLayout {
    std::vector<int64_t> off;
    std::vector<int32_t> pdoc;
    std::vector<uint16_t> ptf;
};
void sparse_sort(const SparseStore* sp, bool moved_only, int vocab, int64_t n_post, HostLayout* out) {
    out->off.assign((size_t)vocab + 1, 0);
    out->pdoc.resize((size_t)n_post);
    out->ptf.resize((size_t)n_post);
    if (moved_only)
        for_each_moved(sp, [&](int64_t d) {
            for (int64_t p = sp->doc_at[d]; p < sp->doc_at[d] + sp->doc_cnt[d]; ++p) out->off[(size_t)sp->h_term[p] + 1]++;
        });
    else
        for (int t = 0; t < vocab; ++t) out->off[(size_t)t + 1] = sp->df[t];
    for (int t = 0; t < vocab; ++t) out->off[(size_t)t + 1] += out->off[t];
    std::vector<int64_t> cur(out->off.begin(), out->off.end() - 1);
    const auto place = [&](int64_t d) {
        for (int64_t p = sp->doc_at[d]; p < sp->doc_at[d] + sp->doc_cnt[d]; ++p) {
            const int64_t at = cur[sp->h_term[p]]++;
            out->pdoc[at] = (int32_t)d;
            out->ptf[at] = sp->h_tf[p];
        }
    };
    if (moved_only) for_each_moved(sp, place);
    else
        for (int64_t d = 0; d < sp->n_docs; ++d) place(d);
}

// the arena back to n_post pairs in document order (nothing changes when memory fails: the old arena stays)
void sparse_squeeze(SparseStore* sp) {
    if ((int64_t)sp->h_term.size() == sp->n_post) return;
    std::vector<int32_t> term;
    std::vector<uint16_t> tf;
    term.reserve((size_t)(sp->n_post + sp->n_post / 8));  // (the slack of arena_reserve: the next set need not move it)
    tf.reserve((size_t)(sp->n_post + sp->n_post / 8));
    for (int64_t d = 0; d < sp->n_docs; ++d) {
        term.insert(term.end(), sp->h_term.begin() + sp->doc_at[d], sp->h_term.begin() + sp->doc_at[d] + sp->doc_cnt[d]);
        tf.insert(tf.end(), sp->h_tf.begin() + sp->doc_at[d], sp->h_tf.begin() + sp->doc_at[d] + sp->doc_cnt[d]);
    }
    int64_t at = 0;
    for (int64_t d = 0; d < sp->n_docs; ++d) {
        sp->doc_at[d] = at;
        at += sp->doc_cnt[d];
    }
    sp->h_term.swap(term);
    sp->h_tf.swap(tf);
}

// The device layout brought up to the host's documents by the first search after a mutation.  While the moved documents'
// postings are at most `sparse_overlay_max_pct` percent of the base's, the base stays and the overlay alone is sorted and
// uploaded; else a full build, after which nothing is moved.  Both upload doc_len and `moved` whole and take a fresh norm
// buffer (avgdl changed).  Every allocation comes before the first swap: a failure leaves the store as it was.
int sparse_upload(mi355dr_index* idx, SparseStore* sp) {
    if (!sp->stale) return MI355DR_OK;
    const bool overlay = sp->has_base && idx->sparse_overlay_max_pct > 0 &&
                         sp->moved_post * 100 <= (int64_t)idx->sparse_overlay_max_pct * sp->base_post;
    HostLayout lay;
    int vocab = (int)sp->vocab;
    try {
        if (overlay) {
            vocab = 0;
            for_each_moved(sp, [&](int64_t d) {
                if (sp->doc_cnt[d]) vocab = std::max(vocab, sp->h_term[sp->doc_at[d] + sp->doc_cnt[d] - 1] + 1);
            });
            sparse_sort(sp, true, vocab, sp->moved_post, &lay);
        } else {
            sparse_squeeze(sp);
            sparse_sort(sp, false, vocab, sp->n_post, &lay);
        }
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "sparse store: host memory for the term-major layout");
    }
    DevBuf<int64_t> term_off;
    DevBuf<int32_t> post_doc, len_dev;
    DevBuf<uint16_t> post_tf;
    DevBuf<unsigned> moved_dev;
    DevBuf<double> norm;
    HIPCHECK(idx, term_off.grow(lay.off.size() * sizeof(int64_t)));
    HIPCHECK(idx, post_doc.grow(std::max<size_t>(lay.pdoc.size(), 1) * sizeof(int32_t)));
    HIPCHECK(idx, post_tf.grow(std::max<size_t>(lay.ptf.size(), 1) * sizeof(uint16_t)));
    HIPCHECK(idx, len_dev.grow(std::max<size_t>(sp->doc_len.size(), 1) * sizeof(int32_t)));
    HIPCHECK(idx, moved_dev.grow(std::max<size_t>(sp->moved.size(), 1) * sizeof(unsigned)));
    HIPCHECK(idx, norm.grow(std::max<size_t>(sp->doc_len.size(), 1) * sizeof(double)));
    HIPCHECK(idx, hipMemcpy(term_off.p, lay.off.data(), lay.off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (!lay.pdoc.empty()) {
        HIPCHECK(idx, hipMemcpy(post_doc.p, lay.pdoc.data(), lay.pdoc.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHECK(idx, hipMemcpy(post_tf.p, lay.ptf.data(), lay.ptf.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    if (!sp->doc_len.empty()) {
        HIPCHECK(idx, hipMemcpy(len_dev.p, sp->doc_len.data(), sp->doc_len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        if (overlay) HIPCHECK(idx, hipMemcpy(moved_dev.p, sp->moved.data(), sp->moved.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        else HIPCHECK(idx, hipMemset(moved_dev.p, 0, sp->moved.size() * sizeof(unsigned)));
    }
    if (overlay) {
        sp->ov_term_off.swap(term_off);
        sp->ov_post_doc.swap(post_doc);
        sp->ov_post_tf.swap(post_tf);
        sp->ov_vocab = vocab;
        sp->ov_active = true;
        sp->ov_post_dev = sp->moved_post;
        sp->dead_post_dev = sp->dead_post;
        idx->s_sparse_overlay_builds++;
    } else {
        sp->term_off.swap(term_off);
        sp->post_doc.swap(post_doc);
        sp->post_tf.swap(post_tf);
        sp->ov_term_off.release();
        sp->ov_post_doc.release();
        sp->ov_post_tf.release();
        std::fill(sp->moved.begin(), sp->moved.end(), 0u);
        sp->has_base = true;
        sp->base_post = sp->n_post;
        sp->base_vocab = vocab;
        sp->moved_post = sp->dead_post = 0;
        sp->ov_vocab = 0;
        sp->ov_active = false;
        sp->ov_post_dev = sp->dead_post_dev = 0;
        idx->s_sparse_full_builds++;
    }
    sp->len_dev.swap(len_dev);
    sp->moved_dev.swap(moved_dev);
    sp->moved_words_dev = (int64_t)sp->moved.size();
    sp->norm.swap(norm);
    sp->norm_valid = false;
    sp->stale = false;
    return MI355DR_OK;
}

inline int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

struct SparseOut {
    double* dist;
    int64_t* rows;
    bool host;
};

// the block and its overflow pieces launch the same instantiation: <true> exactly while the device layout has moved documents,
// <*, true> exactly for a launch with a tile list (a search within a listed subset)
int launch_score(mi355dr_index* idx, SparseStore* sp, hipStream_t s, const SparseStoreView& view, const SparseOverlayView& ov,
                 const SparseQueries& qs, const SparseLists& ls, const SparseLaunch& l, int nq, double k1p1) {
    const int T = idx->sparse_tile_docs;
    if (l.n_tiles >= 0) {
        const SparseFilterView flt{sp->sub_tiles.p + l.tile_at, sp->sub_bits.p, (sp->n_docs + 31) / 32};
        const dim3 grid((unsigned)l.n_tiles, (unsigned)nq);
        const size_t lds = sparse_score_lds_filtered(T, sp->ov_active, ov.terms_cap);
        if (sp->ov_active)
            hipLaunchKernelGGL((k_sparse_score<true, true>), grid, dim3(kSparseThreads), lds, s, view, ov, qs, ls, l.a0, l.a1, T, k1p1,
                               sp->scored.p, flt);
        else
            hipLaunchKernelGGL((k_sparse_score<false, true>), grid, dim3(kSparseThreads), lds, s, view, ov, qs, ls, l.a0, l.a1, T, k1p1,
                               sp->scored.p, flt);
        idx->s_sparse_subset_tiles += l.n_tiles;
        HIPCHECK(idx, hipGetLastError());
        return MI355DR_OK;
    }
    const int64_t tiles = (l.a1 - 1) / T - l.a0 / T + 1;
    const dim3 grid((unsigned)tiles, (unsigned)nq);
    const SparseFilterView none{nullptr, nullptr, 0};
    if (sp->ov_active)
        hipLaunchKernelGGL(k_sparse_score<true>, grid, dim3(kSparseThreads), sparse_score_lds(T, true, ov.terms_cap), s, view, ov, qs, ls, l.a0,
                           l.a1, T, k1p1, sp->scored.p, none);
    else
        hipLaunchKernelGGL(k_sparse_score<false>, grid, dim3(kSparseThreads), sparse_score_lds(T), s, view, ov, qs, ls, l.a0, l.a1, T, k1p1,
                           sp->scored.p, none);
    HIPCHECK(idx, hipGetLastError());
    return MI355DR_OK;
}

// the statistics a sharded call scores with in place of the store's own: the sums over every shard, passed down as a value
struct SparseGlobal {
    int64_t N;
    double avgdl;  // (double)total_len / (double)N, both global
};

inline uint64_t double_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

// the store of the handle (created when there is none), its device layout and the norms of (k1, b, avgdl) brought up to date --
// avgdl is the store's own, or `glob`'s --; *n: the documents a search runs over (0 while no document has tokens)
int sparse_ready(mi355dr_index* idx, double k1, double b, hipStream_t s, int64_t* n_out, const SparseGlobal* glob = nullptr) {
    if (!idx->sp) {
        idx->sp = new (std::nothrow) SparseStore();
        if (!idx->sp) return fail(idx, MI355DR_E_NOMEM, "sparse store: host memory");
    }
    SparseStore* sp = idx->sp;
    if (sp->n_live > 0) CHECK(sparse_upload(idx, sp));
    const int64_t n = sp->n_live > 0 ? sp->n_docs : 0;
    if (!sp->lds_registered) {
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_sparse_score<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)sparse_score_lds(kSparseTileMax)));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_sparse_score<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)sparse_score_lds(kSparseTileMax, true)));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_sparse_score<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)sparse_score_lds_filtered(kSparseTileMax, false, kSparseTermsMax)));
        HIPCHECK(idx, hipFuncSetAttribute((const void*)k_sparse_score<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)sparse_score_lds_filtered(kSparseTileMax, true, kSparseTermsMax)));
        sp->lds_registered = true;
    }
    const double avgdl = glob ? glob->avgdl : (double)sp->total_len / (double)sp->n_live;
    if (n > 0 && !(sp->norm_valid && sp->norm_k1 == k1 && sp->norm_b == b && sp->norm_avgdl == double_bits(avgdl))) {
        hipLaunchKernelGGL(k_sparse_norms, dim3((unsigned)((n + kSparseThreads - 1) / kSparseThreads)), dim3(kSparseThreads), 0, s,
                           sp->len_dev.p, n, avgdl, k1, b, sp->norm.p);
        HIPCHECK(idx, hipGetLastError());
        sp->norm_valid = true;
        sp->norm_k1 = k1;
        sp->norm_b = b;
        sp->norm_avgdl = double_bits(avgdl);
    }
    *n_out = n;
    return MI355DR_OK;
}

// queries [b0, b0 + nb) of the call to the device, in stream order behind the previous block (the host vectors stay as they
// are until the block's last wait); *terms_cap: the block's longest query, even -- the size of the LDS slice tables of every
// k_sparse_score but <false>
int sparse_put_queries(mi355dr_index* idx, SparseStore* sp, const std::vector<int32_t>& terms, const std::vector<double>& weights,
                       const std::vector<int32_t>& offsets, int b0, int nb, hipStream_t s, std::vector<int32_t>& off_block,
                       int* terms_cap, size_t* nt_out) {
    const int32_t t_lo = offsets[b0], t_hi = offsets[b0 + nb];
    const size_t nt = (size_t)(t_hi - t_lo);
    off_block.resize((size_t)nb + 1);
    for (int i = 0; i <= nb; ++i) off_block[i] = offsets[b0 + i] - t_lo;
    *terms_cap = 2;
    for (int i = 0; i < nb; ++i) *terms_cap = std::max(*terms_cap, (offsets[b0 + i + 1] - offsets[b0 + i] + 1) & ~1);
    HIPCHECK(idx, grow_each(std::max<size_t>(nt, 1), sp->q_terms));
    HIPCHECK(idx, grow_each(std::max<size_t>(nt, 1), sp->q_w));
    if (nt) {
        HIPCHECK(idx, hipMemcpyAsync(sp->q_terms.p, terms.data() + t_lo, nt * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHECK(idx, hipMemcpyAsync(sp->q_w.p, weights.data() + t_lo, nt * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIPCHECK(idx, hipMemcpyAsync(sp->q_off.p, off_block.data(), off_block.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    *nt_out = nt;
    return MI355DR_OK;
}

// ---- the sharded forms' collectives (one at a time, in stream order; every rank enters each of them) -------------------------
// the send / receive buffers for a payload of `words` int64 per rank (before the collective they serve)
int sparse_shard_reserve(mi355dr_index* idx, SparseStore* sp, size_t words) {
    HIPCHECK(idx, grow_each(std::max<size_t>(words, 1), sp->sh_send));
    HIPCHECK(idx, grow_each(std::max<size_t>(words, 1) * (size_t)idx->comm_world, sp->sh_recv));
    return MI355DR_OK;
}

// one all-gather: the payload final and visible first (a host transport reads it with copies of its own), a transport error
// returned after the stream is drained
int sparse_gather(mi355dr_index* idx, SparseStore* sp, hipStream_t s, size_t words) {
    HIPCHECK(idx, hipStreamSynchronize(s));
    const int rc = comm_all_gather(idx, sp->sh_send.p, sp->sh_recv.p, words * sizeof(int64_t), s);
    if (rc != MI355DR_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    idx->s_shard_gather_bytes += (int64_t)idx->comm_world * (int64_t)(words * sizeof(int64_t));
    return MI355DR_OK;
}

// a block's kept lists as this rank's packed [2, nb, k] block, one all-gather, the world * k -> k merge into od / orow [nb, k]
int sparse_shard_block(mi355dr_index* idx, SparseStore* sp, hipStream_t s, int nb, int k, double* od, int64_t* orow) {
    const int64_t n_best = (int64_t)nb * k;
    hipLaunchKernelGGL(k_sparse_final_packed, dim3((unsigned)((n_best + kSparseThreads - 1) / kSparseThreads)), dim3(kSparseThreads), 0, s,
                       sp->best_key.p, sp->best_doc.p, n_best, idx->row_offset, sp->sh_send.p);
    HIPCHECK(idx, hipGetLastError());
    CHECK(sparse_gather(idx, sp, s, (size_t)(2 * n_best)));
    return merge_topk_packed(idx, sp->sh_recv.p, idx->comm_world, nb, k, od, orow, s);
}

// The statistics of a call: this rank's [2 + T] payload (n_live, total_len, df of `terms`) uploaded, gathered, summed on the
// device by k_sparse_stats_fold and downloaded into `folded` -- the same integers on every rank.  Creates the store when the
// handle has none (a rank that never added a document still enters the collective).
int sparse_shard_stats(mi355dr_index* idx, hipStream_t s, const std::vector<int32_t>& terms, std::vector<int64_t>& folded) {
    if (!idx->sp) {
        idx->sp = new (std::nothrow) SparseStore();
        if (!idx->sp) return fail(idx, MI355DR_E_NOMEM, "sparse store: host memory");
    }
    SparseStore* sp = idx->sp;
    std::vector<int64_t> payload;
    try {
        shard_stats_payload(sp->n_live, sp->total_len, terms,
                            [&](int32_t t) -> int64_t { return (int64_t)t < sp->vocab ? sp->df[(size_t)t] : 0; }, payload);
        folded.resize(payload.size());
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "sharded sparse search: host memory for the statistics");
    }
    const size_t words = payload.size();
    CHECK(sparse_shard_reserve(idx, sp, words));
    HIPCHECK(idx, grow_each(words, sp->sh_fold));
    HIPCHECK(idx, hipMemcpyAsync(sp->sh_send.p, payload.data(), words * sizeof(int64_t), hipMemcpyHostToDevice, s));
    CHECK(sparse_gather(idx, sp, s, words));
    hipLaunchKernelGGL(k_sparse_stats_fold, dim3((unsigned)((words + kSparseThreads - 1) / kSparseThreads)), dim3(kSparseThreads), 0, s,
                       (const int64_t*)sp->sh_recv.p, (int64_t)words, idx->comm_world, sp->sh_fold.p);
    HIPCHECK(idx, hipGetLastError());
    HIPCHECK(idx, hipMemcpyAsync(folded.data(), sp->sh_fold.p, words * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(idx, hipStreamSynchronize(s));
    return MI355DR_OK;
}

// the lists of a call within a listed subset
struct SparseSubsetArg {
    const int64_t* doc_ids;  // HOST, global ids
    int64_t m;
};

// Queries [0, B) as flat host arrays -- every query's terms ascending, distinct, inside [0, 2^20), at most kSparseTermsMax --
// against the store; results to `out` ([B, k], host or device).  The handle's mutex is held.  `sub`: null, or the list the
// search is restricted to -- its local documents run through k_sparse_pairs when they are at most "sparse_subset_pairs_max",
// else through the launches of sparse_plan_subset with a tile list each.  `glob`: null, or the call is a sharded one (device
// results; the weights were computed from `glob`, the norms are) -- a block's kept lists then leave through sparse_shard_block
// in place of k_sparse_final, and the call counts as a sharded one.
int sparse_search_sorted(mi355dr_index* idx, const std::vector<int32_t>& terms, const std::vector<double>& weights,
                         const std::vector<int32_t>& offsets, int B, int k, double k1, double b, SparseOut out, hipStream_t s,
                         const SparseSubsetArg* sub = nullptr, const SparseGlobal* glob = nullptr) {
    if (glob) idx->s_shard_sparse_searches++;
    else if (sub) idx->s_sparse_subset_searches++;
    else idx->s_sparse_searches++;
    idx->s_sparse_queries += B;
    if (B == 0) return MI355DR_OK;
    int64_t n = 0;
    CHECK(sparse_ready(idx, k1, b, s, &n, glob));
    SparseStore* sp = idx->sp;
    const int cap = idx->sparse_cand_cap;
    std::vector<int32_t> listed;  // the list's local documents, ascending, each once
    std::vector<unsigned> bits;
    SparseLaunchPlan plan;
    bool pairs = false;
    try {
        if (sub) {
            // a list that may take the pair pass is short: sort it; a longer one goes through the bitmap it needs anyway
            const int64_t pairs_max = std::min<int64_t>(idx->sparse_subset_pairs_max, cap);
            if (sub->m <= pairs_max || n == 0) subset_prepare_ids(sub->doc_ids, sub->m, idx->row_offset, n, listed);
            else sparse_subset_scan(sub->doc_ids, sub->m, idx->row_offset, n, listed, bits);
            pairs = (int64_t)listed.size() <= pairs_max;  // (duplicates may have made a longer list short)
            if (pairs) bits.clear();
            else plan = sparse_plan_subset(listed, k, cap, idx->sparse_tile_docs);
        } else {
            plan = sparse_plan_all(n, k, cap);
        }
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "sparse search: host memory for the launch plan");
    }
    if (listed.empty()) pairs = false;  // (nothing to look up: every line is NaN / -1)
    const int n_chunks = pairs ? 1 : (int)plan.ranges.size();
    const int nb_max = std::min(B, kQBlockMax);
    const int np_max = pow2_at_least(k + cap);
    // every buffer of the call before its first launch: a failure leaves the store as it was
    if (pairs) HIPCHECK(idx, grow_each(listed.size(), sp->sub_ids));
    if (!bits.empty()) HIPCHECK(idx, grow_each(bits.size(), sp->sub_bits));
    if (!plan.tiles.empty()) HIPCHECK(idx, grow_each(plan.tiles.size(), sp->sub_tiles));
    HIPCHECK(idx, grow_each((size_t)nb_max * k, sp->best_key, sp->best_doc));
    HIPCHECK(idx, grow_each((size_t)nb_max * cap, sp->cand_key, sp->cand_doc));
    HIPCHECK(idx, grow_each((size_t)nb_max, sp->count));
    HIPCHECK(idx, grow_each((size_t)nb_max + 1, sp->q_off));
    HIPCHECK(idx, grow_each((size_t)nb_max * (std::max(n_chunks, 1) + 1), sp->flags, sp->qlist));
    HIPCHECK(idx, grow_each(1, sp->scored));
    if (out.host) HIPCHECK(idx, grow_each((size_t)nb_max * k, sp->out_dist, sp->out_rows));
    if (glob) CHECK(sparse_shard_reserve(idx, sp, (size_t)2 * nb_max * k));
    HIPCHECK(idx, hipMemsetAsync(sp->scored.p, 0, sizeof(unsigned long long), s));
    // (the list's device forms stay as they are for every block of the call; the host vectors until the first block's wait)
    if (pairs) HIPCHECK(idx, hipMemcpyAsync(sp->sub_ids.p, listed.data(), listed.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (!bits.empty()) HIPCHECK(idx, hipMemcpyAsync(sp->sub_bits.p, bits.data(), bits.size() * sizeof(unsigned), hipMemcpyHostToDevice, s));
    if (!plan.tiles.empty())
        HIPCHECK(idx, hipMemcpyAsync(sp->sub_tiles.p, plan.tiles.data(), plan.tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));

    const SparseStoreView view{sp->term_off.p, sp->post_doc.p, sp->post_tf.p, sp->norm.p, sp->base_vocab};
    SparseOverlayView ov{sp->moved_dev.p, sp->ov_term_off.p, sp->ov_post_doc.p, sp->ov_post_tf.p, sp->moved_words_dev, sp->ov_vocab, 2};
    const double k1p1 = k1 + 1.0;
    std::vector<int32_t> off_block;
    std::vector<int> flags_host, redo_q;
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        size_t nt = 0;
        CHECK(sparse_put_queries(idx, sp, terms, weights, offsets, b0, nb, s, off_block, &ov.terms_cap, &nt));

        SparseLists ls{sp->best_key.p, sp->best_doc.p, sp->cand_key.p, sp->cand_doc.p, sp->count.p, k, cap};
        SparseQueries qs{sp->q_terms.p, sp->q_w.p, sp->q_off.p, nullptr};
        const int64_t n_best = (int64_t)nb * k, n_flags = (int64_t)nb * (n_chunks + 1);
        const int64_t n_reset = std::max(n_best, n_flags);
        hipLaunchKernelGGL(k_sparse_reset, dim3((unsigned)((n_reset + kSparseThreads - 1) / kSparseThreads)), dim3(kSparseThreads), 0, s,
                           sp->best_key.p, sp->best_doc.p, n_best, sp->count.p, (int64_t)nb, sp->flags.p, n_flags);
        HIPCHECK(idx, hipGetLastError());
        if (nt > 0 && pairs) {  // (at most cap listed documents: the lists cannot overflow)
            const SparsePairs pr{sp->sub_ids.p, (int64_t)listed.size(), 0, nullptr, 0, sp->ov_active ? 1 : 0};
            hipLaunchKernelGGL(k_sparse_pairs, dim3((unsigned)((listed.size() + kSparseThreads - 1) / kSparseThreads), (unsigned)nb),
                               dim3(kSparseThreads), 0, s, view, ov, qs, ls, pr, k1p1, sp->scored.p);
            HIPCHECK(idx, hipGetLastError());
            idx->s_sparse_subset_pairs += (int64_t)nb * (int64_t)listed.size();
            hipLaunchKernelGGL(k_sparse_merge, dim3((unsigned)nb), dim3(kSparseThreads), sparse_merge_lds(np_max), s, ls,
                               (const int*)nullptr, np_max, sp->flags.p);
            HIPCHECK(idx, hipGetLastError());
        } else if (nt > 0) {
            for (int c = 0; c < n_chunks; ++c) {
                CHECK(launch_score(idx, sp, s, view, ov, qs, ls, plan.ranges[c], nb, k1p1));
                hipLaunchKernelGGL(k_sparse_merge, dim3((unsigned)nb), dim3(kSparseThreads), sparse_merge_lds(np_max), s, ls,
                                   (const int*)nullptr, np_max, sp->flags.p + (size_t)c * nb);
                HIPCHECK(idx, hipGetLastError());
            }
            if (n_chunks > 1) {  // (the first launch cannot overflow)
                flags_host.resize((size_t)n_chunks * nb);
                HIPCHECK(idx, hipMemcpyAsync(flags_host.data(), sp->flags.p, flags_host.size() * sizeof(int), hipMemcpyDeviceToHost, s));
                HIPCHECK(idx, hipStreamSynchronize(s));
                int* spare = sp->flags.p + (size_t)n_chunks * nb;  // the pieces' flags: must stay zero
                for (int c = 1; c < n_chunks; ++c) {
                    redo_q.clear();
                    for (int q = 0; q < nb; ++q)
                        if (flags_host[(size_t)c * nb + q]) redo_q.push_back(q);
                    if (redo_q.empty()) continue;
                    idx->s_sparse_overflows += (int64_t)redo_q.size();
                    int* ql = sp->qlist.p + (size_t)c * nb;
                    HIPCHECK(idx, hipMemcpyAsync(ql, redo_q.data(), redo_q.size() * sizeof(int), hipMemcpyHostToDevice, s));
                    SparseQueries qr = qs;
                    qr.qlist = ql;
                    for (const SparseLaunch& piece : plan.pieces[c]) {
                        CHECK(launch_score(idx, sp, s, view, ov, qr, ls, piece, (int)redo_q.size(), k1p1));
                        hipLaunchKernelGGL(k_sparse_merge, dim3((unsigned)redo_q.size()), dim3(kSparseThreads), sparse_merge_lds(np_max),
                                           s, ls, (const int*)ql, np_max, spare);
                        HIPCHECK(idx, hipGetLastError());
                    }
                    // a piece holds at most `cap` documents: a flag here is a defect, not an overflow
                    HIPCHECK(idx, hipMemcpyAsync(flags_host.data(), spare, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
                    HIPCHECK(idx, hipStreamSynchronize(s));
                    for (int q = 0; q < nb; ++q)
                        if (flags_host[q]) return fail(idx, MI355DR_E_INTERNAL, "sparse search: a piece of at most cap documents overflowed");
                }
            }
        }
        if (glob) {
            CHECK(sparse_shard_block(idx, sp, s, nb, k, out.dist + (int64_t)b0 * k, out.rows + (int64_t)b0 * k));
            HIPCHECK(idx, hipStreamSynchronize(s));  // (the next block reuses the lists and the payload buffers)
            continue;
        }
        double* od = out.host ? sp->out_dist.p : out.dist + (int64_t)b0 * k;
        int64_t* orow = out.host ? sp->out_rows.p : out.rows + (int64_t)b0 * k;
        hipLaunchKernelGGL(k_sparse_final, dim3((unsigned)((n_best + kSparseThreads - 1) / kSparseThreads)), dim3(kSparseThreads), 0, s,
                           sp->best_key.p, sp->best_doc.p, n_best, idx->row_offset, od, orow);
        HIPCHECK(idx, hipGetLastError());
        if (out.host) {
            HIPCHECK(idx, hipMemcpyAsync(out.dist + (int64_t)b0 * k, od, (size_t)n_best * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHECK(idx, hipMemcpyAsync(out.rows + (int64_t)b0 * k, orow, (size_t)n_best * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        }
        HIPCHECK(idx, hipStreamSynchronize(s));
    }
    unsigned long long scored = 0;
    HIPCHECK(idx, hipMemcpy(&scored, sp->scored.p, sizeof(scored), hipMemcpyDeviceToHost));
    idx->s_sparse_postings_scored += (int64_t)scored;
    return MI355DR_OK;
}

int check_common(mi355dr_index* idx, const int32_t* q_offsets, int B, int k, double k1, double b, const void* od, const void* orow) {
    if (B < 0 || k <= 0) return fail(idx, MI355DR_E_INVALID, "sparse search: B must be >= 0 and k > 0");
    if (k > kKMax) return fail(idx, MI355DR_E_UNSUPPORTED, "sparse search: k exceeds 1024");
    if (!(k1 >= 0.0) || !std::isfinite(k1)) return fail(idx, MI355DR_E_INVALID, "sparse search: k1 must be finite and >= 0");
    if (!(b >= 0.0 && b <= 1.0)) return fail(idx, MI355DR_E_INVALID, "sparse search: b must be in [0, 1]");
    if (B > 0 && (!q_offsets || !od || !orow)) return fail(idx, MI355DR_E_INVALID, "sparse search: null buffer");
    for (int i = 0; i < B; ++i)
        if (q_offsets[i] < 0 || q_offsets[i + 1] < q_offsets[i])
            return fail(idx, MI355DR_E_INVALID, "sparse search: q_offsets must start at >= 0 and never decrease");
    return MI355DR_OK;
}

// the lock, the device, blocks in flight finished, the stream
int sparse_begin(mi355dr_index* idx, std::unique_lock<std::mutex>& lock, void* stream, hipStream_t* s) {
    lock = std::unique_lock<std::mutex>(idx->mu);
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_searches(idx));
    *s = stream ? (hipStream_t)stream : idx->stream;
    return MI355DR_OK;
}

// the queries of a call as sparse_search_sorted takes them
struct SortedQueries {
    std::vector<int32_t> terms, offsets;
    std::vector<double> weights;
};

// the weighted forms' queries, checked, each one's terms sorted ascending
int weighted_queries(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B,
                     SortedQueries* out) {
    std::vector<int32_t>&terms = out->terms, &offsets = out->offsets;
    std::vector<double>& weights = out->weights;
    try {
        offsets.assign((size_t)B + 1, 0);
        std::vector<std::pair<int32_t, double>> one;
        for (int q = 0; q < B; ++q) {
            const int32_t lo = q_offsets[q], hi = q_offsets[q + 1];
            if (hi > lo && (!q_terms || !q_weights)) return fail(idx, MI355DR_E_INVALID, "sparse search: null query");
            if (hi - lo > kSparseTermsMax) return fail(idx, MI355DR_E_UNSUPPORTED, "sparse search: more than 1024 terms in one query");
            one.clear();
            for (int32_t p = lo; p < hi; ++p) {
                const double w = q_weights[p];
                if (q_terms[p] < 0 || q_terms[p] >= kTermLimit)
                    return fail(idx, MI355DR_E_INVALID, "sparse search: term id outside [0, 2^20)");
                if (!std::isfinite(w) || std::fabs(w) > 1e30)
                    return fail(idx, MI355DR_E_INVALID, "sparse search: weights must be finite with |w| <= 1e30");
                one.emplace_back(q_terms[p], w);
            }
            std::sort(one.begin(), one.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            for (size_t i = 1; i < one.size(); ++i)
                if (one[i].first == one[i - 1].first) return fail(idx, MI355DR_E_INVALID, "sparse search: a term is repeated in one query");
            for (const auto& tw : one) {
                terms.push_back(tw.first);
                weights.push_back(tw.second);
            }
            offsets[(size_t)q + 1] = (int32_t)terms.size();
        }
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "sparse search: host memory");
    }
    return MI355DR_OK;
}

// the BM25 forms' queries: raw tokens -> the terms that occur, each once, ascending, weighted by the store's N and df
int bm25_queries(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, SortedQueries* out) {
    const SparseStore* sp = idx->sp;
    const int64_t N = sp ? sp->n_live : 0, vocab = sp ? sp->vocab : 0;
    std::vector<int32_t>&terms = out->terms, &offsets = out->offsets;
    std::vector<int32_t> one;
    std::vector<double>& weights = out->weights;
    try {
        offsets.assign((size_t)B + 1, 0);
        for (int q = 0; q < B; ++q) {
            const int32_t lo = q_offsets[q], hi = q_offsets[q + 1];
            if (hi > lo && !q_tokens) return fail(idx, MI355DR_E_INVALID, "bm25 search: null query");
            one.assign(q_tokens + lo, q_tokens + hi);
            std::sort(one.begin(), one.end());
            one.erase(std::unique(one.begin(), one.end()), one.end());
            if ((int64_t)one.size() > kSparseTermsMax)
                return fail(idx, MI355DR_E_UNSUPPORTED, "bm25 search: more than 1024 distinct terms in one query");
            for (const int32_t t : one) {
                if (t < 0 || t >= vocab) continue;
                const int64_t df = sp->df[t];
                if (df == 0) continue;
                terms.push_back(t);
                weights.push_back(std::log(1.0 + (((double)(N - df) + 0.5) / ((double)df + 0.5))));
            }
            offsets[(size_t)q + 1] = (int32_t)terms.size();
        }
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "bm25 search: host memory");
    }
    return MI355DR_OK;
}

// the eight search forms: weighted (q_terms, q_weights) or BM25 (q_terms are raw tokens), host or device results, the whole
// store or a listed subset
int search_impl(mi355dr_index* idx, bool bm25, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B, int k,
                double k1, double b, SparseOut out, void* stream, const SparseSubsetArg* sub = nullptr) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    CHECK(sparse_begin(idx, lock, stream, &s));
    CHECK(check_common(idx, q_offsets, B, k, k1, b, out.dist, out.rows));
    if (sub && (sub->m < 0 || (sub->m > 0 && !sub->doc_ids)))
        return fail(idx, MI355DR_E_INVALID, "sparse search within a subset: m must be >= 0 and doc_ids not null");
    SortedQueries q;
    CHECK(bm25 ? bm25_queries(idx, q_terms, q_offsets, B, &q) : weighted_queries(idx, q_terms, q_weights, q_offsets, B, &q));
    return sparse_search_sorted(idx, q.terms, q.weights, q.offsets, B, k, k1, b, out, s, sub);
}

constexpr int64_t kPairsLaunchMax = (int64_t)1 << 22;  // (query, document) pairs of one k_sparse_pairs launch of the score forms

// the checks of both score forms, local and sharded (no k and no result lists here)
int check_score(mi355dr_index* idx, const int32_t* q_offsets, int B, double k1, double b, const int64_t* doc_ids, int m,
                const double* out_dist) {
    CHECK(check_common(idx, q_offsets, B, 1, k1, b, idx, idx));
    if (m < 0) return fail(idx, MI355DR_E_INVALID, "sparse scores: m must be >= 0");
    if (B > 0 && m > 0 && (!doc_ids || !out_dist)) return fail(idx, MI355DR_E_INVALID, "sparse scores: null buffer");
    if ((int64_t)B * m > INT32_MAX) return fail(idx, MI355DR_E_UNSUPPORTED, "sparse scores: B * m must be below 2^31");
    return MI355DR_OK;
}

// Queries [0, B) as sparse_search_sorted takes them, B > 0, each against its own row of doc_ids [B, m > 0], through
// k_sparse_pairs in launches of whole rows (or, for a row longer than a launch, parts of one row) staged in buffers of at most
// kPairsLaunchMax.  `glob`: null, or the call is a sharded one -- every launch's distances (NaN where this shard does not hold
// the document; all NaN from a shard without documents) are gathered and folded by k_sparse_fold_scores to the owner's value.
// The launches depend on B and m alone, so every rank enters the same collectives.
int sparse_score_sorted(mi355dr_index* idx, const SortedQueries& q, int B, double k1, double b, const int64_t* doc_ids, int m,
                        double* out_dist, hipStream_t s, const SparseGlobal* glob = nullptr) {
    int64_t n = 0;
    CHECK(sparse_ready(idx, k1, b, s, &n, glob));
    SparseStore* sp = idx->sp;
    if (glob ? glob->N == 0 : n == 0) {  // no document matches anything (the global N is the same on every rank)
        std::fill(out_dist, out_dist + (int64_t)B * m, std::nan(""));
        return MI355DR_OK;
    }
    const int nb_max = std::min(B, kQBlockMax);
    const int rows_per = m <= kPairsLaunchMax ? (int)std::min<int64_t>(nb_max, kPairsLaunchMax / m) : 1;
    const int64_t cols = std::min<int64_t>(m, kPairsLaunchMax);
    std::vector<int32_t> ids_host, off_block;
    try {
        ids_host.resize((size_t)(rows_per * cols));
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "sparse scores: host memory");
    }
    HIPCHECK(idx, grow_each(ids_host.size(), sp->sub_ids, sp->pair_dist));
    if (glob) CHECK(sparse_shard_reserve(idx, sp, ids_host.size()));
    HIPCHECK(idx, grow_each((size_t)nb_max + 1, sp->q_off));
    HIPCHECK(idx, grow_each(1, sp->scored));
    HIPCHECK(idx, hipMemsetAsync(sp->scored.p, 0, sizeof(unsigned long long), s));

    const SparseStoreView view{sp->term_off.p, sp->post_doc.p, sp->post_tf.p, sp->norm.p, sp->base_vocab};
    const SparseLists no_lists{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    SparseOverlayView ov{sp->moved_dev.p, sp->ov_term_off.p, sp->ov_post_doc.p, sp->ov_post_tf.p, sp->moved_words_dev, sp->ov_vocab, 2};
    const double k1p1 = k1 + 1.0;
    for (int b0 = 0; b0 < B; b0 += kQBlockMax) {
        const int nb = std::min(kQBlockMax, B - b0);
        size_t nt = 0;
        CHECK(sparse_put_queries(idx, sp, q.terms, q.weights, q.offsets, b0, nb, s, off_block, &ov.terms_cap, &nt));
        const SparseQueries qs{sp->q_terms.p, sp->q_w.p, sp->q_off.p, nullptr};
        for (int q0 = 0; q0 < nb; q0 += rows_per) {
            const int nq = std::min(rows_per, nb - q0);
            for (int64_t j0 = 0; j0 < m; j0 += cols) {
                const int64_t mm = std::min<int64_t>(cols, m - j0);
                for (int r = 0; r < nq; ++r) {
                    const int64_t* row = doc_ids + (int64_t)(b0 + q0 + r) * m + j0;
                    for (int64_t j = 0; j < mm; ++j) ids_host[(size_t)(r * mm + j)] = (int32_t)subset_local_row(row[j], idx->row_offset, n);
                }
                const size_t n_pairs = (size_t)(nq * mm);
                HIPCHECK(idx, hipMemcpyAsync(sp->sub_ids.p, ids_host.data(), n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
                const SparsePairs pr{sp->sub_ids.p, mm, mm, glob ? (double*)sp->sh_send.p : sp->pair_dist.p, q0, sp->ov_active ? 1 : 0};
                hipLaunchKernelGGL(k_sparse_pairs, dim3((unsigned)((mm + kSparseThreads - 1) / kSparseThreads), (unsigned)nq),
                                   dim3(kSparseThreads), 0, s, view, ov, qs, no_lists, pr, k1p1, sp->scored.p);
                HIPCHECK(idx, hipGetLastError());
                idx->s_sparse_subset_pairs += (int64_t)n_pairs;
                if (glob) {
                    CHECK(sparse_gather(idx, sp, s, n_pairs));
                    hipLaunchKernelGGL(k_sparse_fold_scores, dim3((unsigned)((n_pairs + kSparseThreads - 1) / kSparseThreads)),
                                       dim3(kSparseThreads), 0, s, (const int64_t*)sp->sh_recv.p, (int64_t)n_pairs, idx->comm_world,
                                       (int64_t*)sp->pair_dist.p);
                    HIPCHECK(idx, hipGetLastError());
                }
                // (rows of the launch are whole, or it is part of one row: contiguous in out_dist either way)
                HIPCHECK(idx, hipMemcpyAsync(out_dist + (int64_t)(b0 + q0) * m + j0, sp->pair_dist.p, n_pairs * sizeof(double),
                                             hipMemcpyDeviceToHost, s));
                HIPCHECK(idx, hipStreamSynchronize(s));  // (ids_host and the two device buffers are free again)
            }
        }
    }
    unsigned long long scored = 0;
    HIPCHECK(idx, hipMemcpy(&scored, sp->scored.p, sizeof(scored), hipMemcpyDeviceToHost));
    idx->s_sparse_postings_scored += (int64_t)scored;
    return MI355DR_OK;
}

// mi355dr_score_sparse_subset / mi355dr_score_bm25_subset
int score_impl(mi355dr_index* idx, bool bm25, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B,
               double k1, double b, const int64_t* doc_ids, int m, double* out_dist) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    CHECK(sparse_begin(idx, lock, nullptr, &s));
    CHECK(check_score(idx, q_offsets, B, k1, b, doc_ids, m, out_dist));
    SortedQueries q;
    CHECK(bm25 ? bm25_queries(idx, q_terms, q_offsets, B, &q) : weighted_queries(idx, q_terms, q_weights, q_offsets, B, &q));
    idx->s_sparse_subset_scores++;
    if (B == 0 || m == 0) return MI355DR_OK;
    return sparse_score_sorted(idx, q, B, k1, b, doc_ids, m, out_dist, s);
}

// ---- the six sharded forms (include/mi355dr.h, "row-sharded sparse search") -------------------------------------------------
// What every sharded form starts with, behind the lock: a view refuses, no communicator, then -- after the local form's own
// argument checks, run by `args_ok` -- the merge's sort limit.  Nothing has been touched and no collective entered when one
// fails, and each depends on the arguments and `world` alone.  Behind them the merge's own state is allocated, so that a
// failed allocation, too, comes before the first collective.
template <class ArgCheck>
int sparse_shard_begin(mi355dr_index* idx, const char* what, int width, ArgCheck&& args_ok) {
    if (idx->is_view) return view_refuses(idx, what, /*ask_parent=*/true);
    if (!idx->comm && !idx->comm_custom)
        return fail(idx, MI355DR_E_INVALID, std::string(what) + ": mi355dr_comm_init has not been called on this index");
    CHECK(args_ok());
    if ((int64_t)idx->comm_world * width > kSortMax)
        return fail(idx, MI355DR_E_UNSUPPORTED, std::string(what) + ": world*k exceeds 4096");
    return merge_topk_reserve(idx);  // (what the merge allocates on a handle's first call: ahead of the first collective)
}

// The queries of a sharded call, before its first collective: the weighted forms' queries checked and sorted into `q`; the BM25
// forms' raw tokens checked and their distinct in-range terms collected in `uni` (sparse_shard.h).
int sparse_shard_check_queries(mi355dr_index* idx, bool bm25, const int32_t* q_terms, const double* q_weights,
                               const int32_t* q_offsets, int B, SortedQueries* q, std::vector<int32_t>& uni) {
    if (bm25) {
        for (int i = 0; i < B; ++i)
            if (q_offsets[i + 1] > q_offsets[i] && !q_terms) return fail(idx, MI355DR_E_INVALID, "bm25 search: null query");
        try {
            if (shard_query_terms(q_terms, q_offsets, B, kTermLimit, kSparseTermsMax, uni) >= 0)
                return fail(idx, MI355DR_E_UNSUPPORTED, "bm25 search: more than 1024 distinct terms in one query");
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "bm25 search: host memory");
        }
        return MI355DR_OK;
    }
    return weighted_queries(idx, q_terms, q_weights, q_offsets, B, q);
}

// ... and the statistics they are scored with: ONE gather -- also for a call without any term --, and for BM25 the weights
// from the global N and df.
int sparse_shard_queries(mi355dr_index* idx, bool bm25, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                         int B, hipStream_t s, SortedQueries* q, SparseGlobal* glob) {
    std::vector<int32_t> uni;
    std::vector<int64_t> folded;
    CHECK(sparse_shard_check_queries(idx, bm25, q_terms, q_weights, q_offsets, B, q, uni));
    CHECK(sparse_shard_stats(idx, s, uni, folded));
    glob->N = folded[0];
    glob->avgdl = (double)folded[1] / (double)folded[0];
    if (bm25) {
        try {
            shard_split_weights(q_terms, q_offsets, B, uni, folded.data(), q->terms, q->weights, q->offsets);
        } catch (const std::bad_alloc&) {
            return fail(idx, MI355DR_E_NOMEM, "bm25 search: host memory");
        }
    }
    return MI355DR_OK;
}

int search_sharded_impl(mi355dr_index* idx, const char* what, bool bm25, const int32_t* q_terms, const double* q_weights,
                        const int32_t* q_offsets, int B, int k, double k1, double b, double* out_dist_dev, int64_t* out_rows_dev,
                        void* stream, const SparseSubsetArg* sub = nullptr) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    CHECK(sparse_begin(idx, lock, stream, &s));
    CHECK(sparse_shard_begin(idx, what, k, [&]() -> int {
        CHECK(check_common(idx, q_offsets, B, k, k1, b, out_dist_dev, out_rows_dev));
        if (sub && (sub->m < 0 || (sub->m > 0 && !sub->doc_ids)))
            return fail(idx, MI355DR_E_INVALID, "sparse search within a subset: m must be >= 0 and doc_ids not null");
        return MI355DR_OK;
    }));
    SortedQueries q;
    SparseGlobal glob{0, 0.0};
    if (B == 0) {  // (no collective: every rank passes the same B)
        idx->s_shard_sparse_searches++;
        return MI355DR_OK;
    }
    CHECK(sparse_shard_queries(idx, bm25, q_terms, q_weights, q_offsets, B, s, &q, &glob));
    return sparse_search_sorted(idx, q.terms, q.weights, q.offsets, B, k, k1, b, SparseOut{out_dist_dev, out_rows_dev, false}, s, sub,
                                &glob);
}

int score_sharded_impl(mi355dr_index* idx, const char* what, bool bm25, const int32_t* q_terms, const double* q_weights,
                       const int32_t* q_offsets, int B, double k1, double b, const int64_t* doc_ids, int m, double* out_dist) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    CHECK(sparse_begin(idx, lock, nullptr, &s));
    CHECK(sparse_shard_begin(idx, what, 1, [&]() -> int { return check_score(idx, q_offsets, B, k1, b, doc_ids, m, out_dist); }));
    if (B == 0 || m == 0) {  // (a no-op like the local form's, on every rank: the queries are still checked)
        SortedQueries unused;
        std::vector<int32_t> uni;
        CHECK(sparse_shard_check_queries(idx, bm25, q_terms, q_weights, q_offsets, B, &unused, uni));
        idx->s_shard_sparse_scores++;
        return MI355DR_OK;
    }
    SortedQueries q;
    SparseGlobal glob{0, 0.0};
    CHECK(sparse_shard_queries(idx, bm25, q_terms, q_weights, q_offsets, B, s, &q, &glob));
    idx->s_shard_sparse_scores++;
    return sparse_score_sorted(idx, q, B, k1, b, doc_ids, m, out_dist, s, &glob);
}

// documents [0, n) of a call as terms[offsets[j] .. offsets[j + 1]); offsets null: n documents without tokens
int check_ragged(mi355dr_index* idx, const std::string& what, const int32_t* terms, const int64_t* offsets, int64_t n) {
    if (!offsets) return MI355DR_OK;
    if (offsets[0] < 0) return fail(idx, MI355DR_E_INVALID, what + ": offsets must start at >= 0");
    for (int64_t d = 0; d < n; ++d) {
        if (offsets[d + 1] < offsets[d]) return fail(idx, MI355DR_E_INVALID, what + ": offsets must never decrease");
        if (offsets[d + 1] - offsets[d] > INT32_MAX) return fail(idx, MI355DR_E_UNSUPPORTED, what + ": a document of more than 2^31 - 1 tokens");
    }
    if (offsets[n] > offsets[0] && !terms) return fail(idx, MI355DR_E_INVALID, what + ": null terms");
    return MI355DR_OK;
}

// the documents of a call as sorted (term, tf) pairs: document j is [end[j - 1], end[j]) of term / tf, len[j] its tokens
struct SparseDigest {
    std::vector<int32_t> term, len;
    std::vector<uint16_t> tf;
    std::vector<int64_t> end;
    int64_t max_term = -1;
};
int sparse_digest(mi355dr_index* idx, const std::string& what, const int32_t* terms, const int64_t* offsets, int64_t n, SparseDigest* a) {
    std::vector<int32_t> one;
    a->end.reserve((size_t)n);
    a->len.reserve((size_t)n);
    for (int64_t d = 0; d < n; ++d) {
        one.clear();
        if (offsets) one.assign(terms + offsets[d], terms + offsets[d + 1]);
        std::sort(one.begin(), one.end());
        if (!one.empty() && (one.front() < 0 || one.back() >= kTermLimit))
            return fail(idx, MI355DR_E_INVALID, what + ": term id outside [0, 2^20) in document " + std::to_string(d));
        for (size_t i = 0; i < one.size();) {
            size_t j = i;
            while (j < one.size() && one[j] == one[i]) ++j;
            if (j - i > (size_t)kTfMax)
                return fail(idx, MI355DR_E_UNSUPPORTED, what + ": a term occurs more than 4095 times in document " + std::to_string(d));
            a->term.push_back(one[i]);
            a->tf.push_back((uint16_t)(j - i));
            i = j;
        }
        a->end.push_back((int64_t)a->term.size());
        a->len.push_back((int32_t)one.size());
        if (!one.empty()) a->max_term = std::max<int64_t>(a->max_term, one.back());
    }
    return MI355DR_OK;
}

// room for `more` pairs behind the arena.  When it has to move it takes an eighth more than asked for, and at least half as
// much again as it holds: an exact reserve would copy the whole arena at every call
void arena_reserve(SparseStore* sp, size_t more) {
    const size_t need = sp->h_term.size() + more;
    if (need <= sp->h_term.capacity() && need <= sp->h_tf.capacity()) return;
    const size_t want = std::max(need + need / 8, sp->h_term.size() + sp->h_term.size() / 2);
    sp->h_term.reserve(want);
    sp->h_tf.reserve(want);
}

// Document d becomes document j of the digest; the room (arena, df) is there, so this cannot fail.  Its old pairs stay behind
// in the arena.  False: it had no tokens and gets none -- nothing changes.
bool sparse_put(SparseStore* sp, int64_t d, const SparseDigest& a, int64_t j) {
    const int64_t lo = j ? a.end[(size_t)j - 1] : 0, cnt = a.end[(size_t)j] - lo;
    const int64_t old_at = sp->doc_at[d], old_cnt = sp->doc_cnt[d];
    if (old_cnt == 0 && cnt == 0) return false;
    unsigned& word = sp->moved[(size_t)(d >> 5)];
    const unsigned bit = 1u << (d & 31);
    if (word & bit) {
        sp->moved_post -= old_cnt;
    } else {  // until now its content was the base's (a document appended since the base was built has none there)
        word |= bit;
        sp->dead_post += old_cnt;
    }
    for (int64_t p = old_at; p < old_at + old_cnt; ++p) sp->df[sp->h_term[p]]--;
    sp->n_post -= old_cnt;
    sp->total_len -= sp->doc_len[d];
    sp->n_live -= sp->doc_len[d] > 0;
    sp->doc_at[d] = (int64_t)sp->h_term.size();
    sp->doc_cnt[d] = (int32_t)cnt;
    sp->doc_len[d] = a.len[(size_t)j];
    sp->h_term.insert(sp->h_term.end(), a.term.begin() + lo, a.term.begin() + lo + cnt);
    sp->h_tf.insert(sp->h_tf.end(), a.tf.begin() + lo, a.tf.begin() + lo + cnt);
    for (int64_t p = lo; p < lo + cnt; ++p) sp->df[a.term[(size_t)p]]++;
    sp->n_post += cnt;
    sp->moved_post += cnt;
    sp->total_len += a.len[(size_t)j];
    sp->n_live += a.len[(size_t)j] > 0;
    if (cnt) sp->vocab = std::max<int64_t>(sp->vocab, (int64_t)a.term[(size_t)(lo + cnt - 1)] + 1);
    while (sp->vocab > 0 && sp->df[(size_t)sp->vocab - 1] == 0) --sp->vocab;
    return true;
}

// mi355dr_set_sparse, and mi355dr_remove_sparse as the set of n empty sequences (offsets null)
int set_sparse_impl(mi355dr_index* idx, const std::string& what, const int64_t* doc_ids, const int32_t* terms, const int64_t* offsets,
                    int64_t n) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, what.c_str());
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_searches(idx));
    const bool removing = what == "remove_sparse";
    if (n < 0) return fail(idx, MI355DR_E_INVALID, what + ": n must be >= 0");
    if (n == 0) return MI355DR_OK;
    if (!doc_ids || (!removing && !offsets)) return fail(idx, MI355DR_E_INVALID, what + ": null buffer");
    CHECK(check_ragged(idx, what, terms, offsets, n));
    SparseStore* sp = idx->sp;
    const int64_t have = sp ? sp->n_docs : 0;
    try {
        std::vector<int64_t> ids(doc_ids, doc_ids + n);
        std::sort(ids.begin(), ids.end());
        if (ids.front() < 0 || ids.back() >= have)
            return fail(idx, MI355DR_E_INVALID, what + ": a document id outside [0, " + std::to_string(have) + ")");
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end())
            return fail(idx, MI355DR_E_INVALID, what + ": a document id is listed twice");
        SparseDigest a;
        CHECK(sparse_digest(idx, what, terms, offsets, n, &a));
        // room first: what follows cannot fail
        arena_reserve(sp, a.term.size());
        if ((size_t)(a.max_term + 1) > sp->df.size()) sp->df.resize((size_t)(a.max_term + 1), 0);
        for (int64_t j = 0; j < n; ++j)
            if (sparse_put(sp, doc_ids[j], a, j)) sp->stale = true;
        idx->s_sparse_sets += n;
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, what + ": host memory");
    }
    return MI355DR_OK;
}

}  // namespace

extern "C" {

int mi355dr_add_sparse(mi355dr_index* idx, const int32_t* terms, const int64_t* offsets, int64_t n_docs) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (idx->is_view) return view_refuses(idx, "add_sparse");
    HIPCHECK(idx, hipSetDevice(idx->device));
    CHECK(drain_searches(idx));
    if (n_docs < 0 || !offsets) return fail(idx, MI355DR_E_INVALID, "add_sparse: n_docs must be >= 0 and offsets not null");
    CHECK(check_ragged(idx, "add_sparse", terms, offsets, n_docs));
    const int64_t have = idx->sp ? idx->sp->n_docs : 0;
    if (have + n_docs > kDocsMax) return fail(idx, MI355DR_E_UNSUPPORTED, "add_sparse: more than 2^31 - 2 documents");
    if (n_docs == 0) return MI355DR_OK;
    try {
        // the new documents as sorted (term, tf) pairs, checked, before anything of the store changes
        SparseDigest a;
        CHECK(sparse_digest(idx, "add_sparse", terms, offsets, n_docs, &a));
        if (!idx->sp) idx->sp = new SparseStore();
        SparseStore* sp = idx->sp;
        // room first: what follows cannot fail
        const size_t docs = (size_t)(sp->n_docs + n_docs);
        sp->doc_len.reserve(docs);
        sp->doc_at.reserve(docs);
        sp->doc_cnt.reserve(docs);
        sp->moved.reserve((docs + 31) / 32);
        arena_reserve(sp, a.term.size());
        if ((size_t)(a.max_term + 1) > sp->df.size()) sp->df.resize((size_t)(a.max_term + 1), 0);
        sp->moved.resize((docs + 31) / 32, 0u);
        for (int64_t j = 0; j < n_docs; ++j) {  // (an appended document is not in the base: it rides the overlay or waits for a full build)
            sp->doc_len.push_back(0);
            sp->doc_at.push_back(0);
            sp->doc_cnt.push_back(0);
            sparse_put(sp, sp->n_docs++, a, j);
        }
        sp->stale = true;
    } catch (const std::bad_alloc&) {
        return fail(idx, MI355DR_E_NOMEM, "add_sparse: host memory");
    }
    return MI355DR_OK;
}

int mi355dr_set_sparse(mi355dr_index* idx, const int64_t* doc_ids, const int32_t* terms, const int64_t* offsets, int64_t n) {
    return set_sparse_impl(idx, "set_sparse", doc_ids, terms, offsets, n);
}

int mi355dr_remove_sparse(mi355dr_index* idx, const int64_t* doc_ids, int64_t n) {
    return set_sparse_impl(idx, "remove_sparse", doc_ids, nullptr, nullptr, n);
}

int64_t mi355dr_live_sparse(const mi355dr_index* idx) { return idx && idx->sp ? idx->sp->n_live : 0; }

int64_t mi355dr_size_sparse(const mi355dr_index* idx) { return idx && idx->sp ? idx->sp->n_docs : 0; }

int mi355dr_sparse_df(mi355dr_index* idx, const int32_t* terms, int64_t n, int64_t* out_df) {
    if (!idx) return fail(nullptr, MI355DR_E_INVALID, "null index");
    std::lock_guard<std::mutex> g(idx->mu);
    if (n < 0 || (n > 0 && (!terms || !out_df))) return fail(idx, MI355DR_E_INVALID, "sparse_df: bad arguments");
    const SparseStore* sp = idx->sp;
    for (int64_t i = 0; i < n; ++i) out_df[i] = sp && terms[i] >= 0 && terms[i] < sp->vocab ? sp->df[terms[i]] : 0;
    return MI355DR_OK;
}

int mi355dr_search_sparse(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B, int k,
                          double k1, double b, double* out_dist, int64_t* out_rows) {
    return search_impl(idx, false, q_terms, q_weights, q_offsets, B, k, k1, b, SparseOut{out_dist, out_rows, true}, nullptr);
}
int mi355dr_search_sparse_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B,
                                 int k, double k1, double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return search_impl(idx, false, q_terms, q_weights, q_offsets, B, k, k1, b, SparseOut{out_dist_dev, out_rows_dev, false}, stream);
}
int mi355dr_search_bm25(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1, double b,
                        double* out_dist, int64_t* out_rows) {
    return search_impl(idx, true, q_tokens, nullptr, q_offsets, B, k, k1, b, SparseOut{out_dist, out_rows, true}, nullptr);
}
int mi355dr_search_bm25_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1, double b,
                               double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return search_impl(idx, true, q_tokens, nullptr, q_offsets, B, k, k1, b, SparseOut{out_dist_dev, out_rows_dev, false}, stream);
}

int mi355dr_search_sparse_subset(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B,
                                 int k, double k1, double b, const int64_t* doc_ids, int64_t m, double* out_dist, int64_t* out_rows) {
    const SparseSubsetArg sub{doc_ids, m};
    return search_impl(idx, false, q_terms, q_weights, q_offsets, B, k, k1, b, SparseOut{out_dist, out_rows, true}, nullptr, &sub);
}
int mi355dr_search_sparse_subset_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                        int B, int k, double k1, double b, const int64_t* doc_ids, int64_t m, double* out_dist_dev,
                                        int64_t* out_rows_dev, void* stream) {
    const SparseSubsetArg sub{doc_ids, m};
    return search_impl(idx, false, q_terms, q_weights, q_offsets, B, k, k1, b, SparseOut{out_dist_dev, out_rows_dev, false}, stream, &sub);
}
int mi355dr_search_bm25_subset(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1, double b,
                               const int64_t* doc_ids, int64_t m, double* out_dist, int64_t* out_rows) {
    const SparseSubsetArg sub{doc_ids, m};
    return search_impl(idx, true, q_tokens, nullptr, q_offsets, B, k, k1, b, SparseOut{out_dist, out_rows, true}, nullptr, &sub);
}
int mi355dr_search_bm25_subset_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1,
                                      double b, const int64_t* doc_ids, int64_t m, double* out_dist_dev, int64_t* out_rows_dev,
                                      void* stream) {
    const SparseSubsetArg sub{doc_ids, m};
    return search_impl(idx, true, q_tokens, nullptr, q_offsets, B, k, k1, b, SparseOut{out_dist_dev, out_rows_dev, false}, stream, &sub);
}
int mi355dr_score_sparse_subset(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets, int B,
                                double k1, double b, const int64_t* doc_ids, int m, double* out_dist) {
    return score_impl(idx, false, q_terms, q_weights, q_offsets, B, k1, b, doc_ids, m, out_dist);
}
int mi355dr_score_bm25_subset(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, double k1, double b,
                              const int64_t* doc_ids, int m, double* out_dist) {
    return score_impl(idx, true, q_tokens, nullptr, q_offsets, B, k1, b, doc_ids, m, out_dist);
}

int mi355dr_search_sparse_sharded_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                         int B, int k, double k1, double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return search_sharded_impl(idx, "search_sparse_sharded_device", false, q_terms, q_weights, q_offsets, B, k, k1, b, out_dist_dev,
                               out_rows_dev, stream);
}
int mi355dr_search_bm25_sharded_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k, double k1,
                                       double b, double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    return search_sharded_impl(idx, "search_bm25_sharded_device", true, q_tokens, nullptr, q_offsets, B, k, k1, b, out_dist_dev,
                               out_rows_dev, stream);
}
int mi355dr_search_sparse_subset_sharded_device(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights,
                                                const int32_t* q_offsets, int B, int k, double k1, double b, const int64_t* doc_ids,
                                                int64_t m, double* out_dist_dev, int64_t* out_rows_dev, void* stream) {
    const SparseSubsetArg sub{doc_ids, m};
    return search_sharded_impl(idx, "search_sparse_subset_sharded_device", false, q_terms, q_weights, q_offsets, B, k, k1, b,
                               out_dist_dev, out_rows_dev, stream, &sub);
}
int mi355dr_search_bm25_subset_sharded_device(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, int k,
                                              double k1, double b, const int64_t* doc_ids, int64_t m, double* out_dist_dev,
                                              int64_t* out_rows_dev, void* stream) {
    const SparseSubsetArg sub{doc_ids, m};
    return search_sharded_impl(idx, "search_bm25_subset_sharded_device", true, q_tokens, nullptr, q_offsets, B, k, k1, b, out_dist_dev,
                               out_rows_dev, stream, &sub);
}
int mi355dr_score_sparse_subset_sharded(mi355dr_index* idx, const int32_t* q_terms, const double* q_weights, const int32_t* q_offsets,
                                        int B, double k1, double b, const int64_t* doc_ids, int m, double* out_dist) {
    return score_sharded_impl(idx, "score_sparse_subset_sharded", false, q_terms, q_weights, q_offsets, B, k1, b, doc_ids, m, out_dist);
}
int mi355dr_score_bm25_subset_sharded(mi355dr_index* idx, const int32_t* q_tokens, const int32_t* q_offsets, int B, double k1, double b,
                                      const int64_t* doc_ids, int m, double* out_dist) {
    return score_sharded_impl(idx, "score_bm25_subset_sharded", true, q_tokens, nullptr, q_offsets, B, k1, b, doc_ids, m, out_dist);
}

}  // extern "C"
