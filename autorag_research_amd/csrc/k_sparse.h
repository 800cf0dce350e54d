// k_sparse.h -- BM25 / weighted sparse scoring over a term-major posting store.
//
// The arithmetic is the contract of include/mi355dr.h ("sparse store"): IEEE double, one rounding per operation, a document's
// sum taken over the query's terms in ASCENDING term id.  Three kernels serve one block of <= kQBlockMax queries:
//   k_sparse_norms   norm_i = k1 * ((1 - b) + b * (L_i / avgdl)) for every document, once per (k1, b, store state)
//   k_sparse_score   one workgroup per (tile of T documents, query): term-at-a-time into LDS accumulators, then the touched
//                    documents that can still enter the query's top-k are appended to its candidate list.  <false>: one
//                    layout, the store as the last full build left it.  <true>: a mutated store -- the base layout minus the
//                    `moved` documents, plus the overlay layout that holds those documents' current postings
//                    <*, true>: the same two within a listed subset -- the launch's tiles come from a list, and a posting of
//                    a document whose `allowed` bit is clear is skipped
//   k_sparse_pairs   one thread per (query, listed document): the document looked up in each of the query's term slices --
//                    the exact scores of a pool, or the matches of a short list appended to the candidate lists
//   k_sparse_merge   one workgroup per query: kept top-k + candidate list sorted under (distance asc, NaN last, id asc)
//   k_sparse_final   the kept lists written out as (distance, id + row_offset), NaN / -1 behind the matches
// The candidate list is the one bounded buffer: appends count past its end, the merge sees the count, drops the WHOLE list of
// that (query, launch) and flags it; the host then runs the launch's document range again for the flagged queries in pieces
// of at most `cap` documents, which cannot overflow.  A list's order is whatever the appends' atomics gave, but the merge
// sorts under a total order and every document is merged once, so the result does not depend on scheduling.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kSparseThreads = 256;
constexpr int kSparseTermsMax = 1024;   // distinct terms of one query
constexpr int kSparseTileMax = 8192;    // documents per LDS tile (64 KiB of accumulators)
constexpr int kSparseCapMax = 2048;     // candidate slots per query: kKMax kept + a full list fit one kSortMax sort
static_assert(kKMax + kSparseCapMax <= kSortMax, "the merge sorts the kept list and a full candidate list together");

// LDS of k_sparse_score: acc[T] doubles | slice start [kSparseTermsMax] int64 | slice length [kSparseTermsMax] int32 |
// touched bitmap [T / 32] | postings counter.  With an overlay: a second slice table behind the first and the tile's `moved`
// bits behind `touched` -- acc | start | overlay start | length | overlay length | touched | moved | counter -- and both
// tables hold `terms_cap` entries, the most terms of a query of the block (even, <= kSparseTermsMax), not kSparseTermsMax:
// two full tables would cost 24 KiB and leave three workgroups per CU at T = 2048 where the one-layout kernel has five
__host__ __device__ inline size_t sparse_score_lds(int T, bool overlay = false, int terms_cap = kSparseTermsMax) {
    const size_t per_term = sizeof(int64_t) + sizeof(int32_t), bits = (size_t)(T / 32) * 4;
    if (!overlay) return (size_t)T * sizeof(double) + (size_t)kSparseTermsMax * per_term + bits + 16;
    return (size_t)T * sizeof(double) + 2 * (size_t)terms_cap * per_term + 2 * bits + 16;
}
// the filtered instantiations: the tile's `allowed` bits behind `touched` / `moved`, and slice tables of `terms_cap` entries in
// both (acc | start | [overlay start] | length | [overlay length] | touched | [moved] | allowed | counter)
__host__ __device__ inline size_t sparse_score_lds_filtered(int T, bool overlay, int terms_cap) {
    const size_t per_term = sizeof(int64_t) + sizeof(int32_t), bits = (size_t)(T / 32) * 4;
    return (size_t)T * sizeof(double) + (overlay ? 2 : 1) * (size_t)terms_cap * per_term + (overlay ? 3 : 2) * bits + 16;
}
__host__ __device__ inline size_t sparse_merge_lds(int np) { return (size_t)np * (sizeof(uint64_t) + sizeof(int32_t)); }

__device__ __forceinline__ bool sparse_before(uint64_t k1, int32_t r1, uint64_t k2, int32_t r2) {
    return k1 < k2 || (k1 == k2 && r1 < r2);
}

// first position in doc[lo, hi) (ascending) that is >= x
__device__ __forceinline__ int64_t sparse_lower_bound(const int32_t* __restrict__ doc, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)doc[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kSparseThreads) void k_sparse_norms(const int32_t* __restrict__ doc_len, int64_t n_docs, double avgdl,
                                                                 double k1, double b, double* __restrict__ norm) {
    const int64_t i = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
    if (i >= n_docs) return;
    const double r = (double)doc_len[i] / avgdl;
    const double x = b * r;
    const double y = (1.0 - b) + x;
    norm[i] = k1 * y;
}

struct SparseStoreView {
    const int64_t* term_off;  // [vocab + 1] postings of term t: [term_off[t], term_off[t + 1])
    const int32_t* post_doc;  // ascending inside a term
    const uint16_t* post_tf;  // 1 .. 4095
    const double* norm;       // [n_docs]
    int vocab;
};
// what a mutated store adds to the base layout: one bit per document whose postings in the base are no longer its content,
// and a second term-major layout of the same format with the current postings of those documents
struct SparseOverlayView {
    const unsigned* moved;    // [moved_words] bit d & 31 of word d >> 5
    const int64_t* term_off;  // [vocab + 1]
    const int32_t* post_doc;  // ascending inside a term; every document here has its moved bit set
    const uint16_t* post_tf;
    int64_t moved_words;
    int vocab;
    int terms_cap;            // entries of each LDS slice table: >= the terms of every query of the launch, even
};
// a search within a listed subset (kFilter): the launch's tiles and one bit per document that is listed
struct SparseFilterView {
    const int32_t* tiles;     // [gridDim.x] tile indices, ascending: tile x of the launch covers [tiles[x] * T, + T)
    const unsigned* allowed;  // [allowed_words] bit d & 31 of word d >> 5
    int64_t allowed_words;
};
struct SparseQueries {
    const int32_t* terms;    // each query's terms ascending, distinct, inside [0, vocab)
    const double* weights;
    const int32_t* offsets;  // [nb + 1]
    const int* qlist;        // null: blockIdx.y is the query; else the launch's queries
};
struct SparseLists {
    uint64_t* best_key;  // [nb, k] kept top-k, sorted; padding (kKeyNaN, kRowNone)
    int32_t* best_doc;
    uint64_t* cand_key;  // [nb, cap]
    int32_t* cand_doc;
    unsigned* count;     // [nb] appends of the launch in progress (may pass cap)
    int k, cap;
};

// grid: (tiles of the launch, queries of the launch).  The launch covers documents [a0, a1); tile x covers
// [(a0 / T + x) * T, + T) cut to [a0, a1).  T: a power of two, 256 .. kSparseTileMax.
// kOverlay: `ov` is read (else it is ignored and the kernel is the one-layout kernel).  Within one term the base postings that
// survive (document not moved) and the overlay's postings (documents moved) name disjoint documents, so the accumulation stays
// plain read-add-writes; a skipped posting is neither added nor counted, so an emptied document is never touched.
// kFilter: `flt` is read (else it is ignored).  Tile x is tile flt.tiles[x], cut to [a0, a1) as before; a posting of a
// document that is not allowed is skipped like a dead one; the slice tables hold ov.terms_cap entries with or without an
// overlay (of `ov`, <false, true> reads terms_cap alone).
template <bool kOverlay, bool kFilter = false>
__global__ __launch_bounds__(kSparseThreads) void k_sparse_score(SparseStoreView st, SparseOverlayView ov, SparseQueries qs,
                                                                 SparseLists ls, int64_t a0, int64_t a1, int T, double k1p1,
                                                                 unsigned long long* __restrict__ postings_scored, SparseFilterView flt) {
    extern __shared__ __align__(16) unsigned char sparse_smem[];
    double* acc = (double*)sparse_smem;
    int64_t* s_lo = (int64_t*)(acc + T);
    const int terms_cap = kOverlay || kFilter ? ov.terms_cap : kSparseTermsMax;
    int64_t* o_lo = s_lo + (kOverlay ? terms_cap : 0);
    int32_t* s_n = (int32_t*)(o_lo + terms_cap);
    int32_t* o_n = s_n + (kOverlay ? terms_cap : 0);
    unsigned* touched = (unsigned*)(o_n + terms_cap);
    unsigned* moved = touched + (kOverlay ? T / 32 : 0);
    unsigned* allowed = moved + (kFilter ? T / 32 : 0);
    unsigned* s_scored = allowed + T / 32;

    const int tid = threadIdx.x;
    const int q = qs.qlist ? qs.qlist[blockIdx.y] : (int)blockIdx.y;
    int64_t t0;
    if constexpr (kFilter) t0 = (int64_t)flt.tiles[blockIdx.x] * T;
    else t0 = (a0 / T + (int64_t)blockIdx.x) * T;
    const int64_t d0 = t0 > a0 ? t0 : a0;
    const int64_t d1 = t0 + T < a1 ? t0 + T : a1;
    const int qo = qs.offsets[q];
    int nt = qs.offsets[q + 1] - qo;
    if (nt > terms_cap) nt = terms_cap;  // (the host refuses a query of more than kSparseTermsMax terms and sizes terms_cap)

    // ---- 1: every term's posting slice inside [d0, d1)
    int any = 0;
    if constexpr (kOverlay) {
        // the two layouts side by side: waves 0 and 1 search the base while waves 2 and 3 search the overlay, so the chain of
        // dependent loads a lane waits for is as long as with one layout
        constexpr int kHalf = kSparseThreads / 2;
        const bool in_ov = tid >= kHalf;  // (wave-uniform)
        const int64_t* __restrict__ term_off = in_ov ? ov.term_off : st.term_off;
        const int32_t* __restrict__ post_doc = in_ov ? ov.post_doc : st.post_doc;
        const int vocab = in_ov ? ov.vocab : st.vocab;
        int64_t* out_lo = in_ov ? o_lo : s_lo;
        int32_t* out_n = in_ov ? o_n : s_n;
        for (int i = tid & (kHalf - 1); i < nt; i += kHalf) {
            const int t = qs.terms[qo + i];
            int64_t lo = 0, hi = 0;
            if (t >= 0 && t < vocab && d0 < d1) {
                const int64_t p0 = term_off[t], p1 = term_off[t + 1];
                lo = sparse_lower_bound(post_doc, p0, p1, d0);
                hi = sparse_lower_bound(post_doc, lo, p1, d1);
            }
            out_lo[i] = lo;
            out_n[i] = (int32_t)(hi - lo);  // <= T
            any |= hi > lo;
        }
    } else {
        for (int i = tid; i < nt; i += kSparseThreads) {
            const int t = qs.terms[qo + i];
            int64_t lo = 0, hi = 0;
            if (t >= 0 && t < st.vocab && d0 < d1) {
                const int64_t p0 = st.term_off[t], p1 = st.term_off[t + 1];
                lo = sparse_lower_bound(st.post_doc, p0, p1, d0);
                hi = sparse_lower_bound(st.post_doc, lo, p1, d1);
            }
            s_lo[i] = lo;
            s_n[i] = (int32_t)(hi - lo);  // <= T
            any |= hi > lo;
        }
    }
    if (!__syncthreads_or(any)) return;  // (block-uniform) nothing of this query in this tile

    // ---- 2: accumulators at +0.0, nothing touched
    for (int j = tid; j < T; j += kSparseThreads) acc[j] = 0.0;
    for (int j = tid; j < T / 32; j += kSparseThreads) touched[j] = 0u;
    if constexpr (kOverlay) {
        const int64_t w0 = t0 >> 5;  // (t0 is a multiple of T >= 256)
        for (int j = tid; j < T / 32; j += kSparseThreads) moved[j] = w0 + j < ov.moved_words ? ov.moved[w0 + j] : 0u;
    }
    if constexpr (kFilter) {
        const int64_t w0 = t0 >> 5;
        for (int j = tid; j < T / 32; j += kSparseThreads) allowed[j] = w0 + j < flt.allowed_words ? flt.allowed[w0 + j] : 0u;
    }
    if (tid == 0) *s_scored = 0u;
    __syncthreads();

    // ---- 3: term at a time, ascending; inside one term every document occurs once, so the read-add-writes never collide,
    // and the barrier between terms makes each document's order of additions the contract's
    unsigned scored = 0;
    for (int i = 0; i < nt; ++i) {
        const int n = s_n[i];  // (block-uniform)
        const int m = kOverlay ? o_n[i] : 0;
        if (n == 0 && m == 0) continue;
        const int64_t lo = s_lo[i];
        const double w = qs.weights[qo + i];
        for (int p = tid; p < n; p += kSparseThreads) {
            const int64_t doc = st.post_doc[lo + p];
            const double tf = (double)st.post_tf[lo + p];
            const int j = (int)(doc - t0);
            if constexpr (kOverlay) {
                if (moved[j >> 5] >> (j & 31) & 1u) continue;  // a dead posting: the document's content is in the overlay
            }
            if constexpr (kFilter) {
                if (!(allowed[j >> 5] >> (j & 31) & 1u)) continue;  // not listed
            }
            const double frac = (tf * k1p1) / (tf + st.norm[doc]);
            acc[j] = acc[j] + (w * frac);
            atomicOr(&touched[j >> 5], 1u << (j & 31));
            ++scored;
        }
        if constexpr (kOverlay) {
            const int64_t olo = o_lo[i];
            for (int p = tid; p < m; p += kSparseThreads) {
                const int64_t doc = ov.post_doc[olo + p];
                const double tf = (double)ov.post_tf[olo + p];
                const int j = (int)(doc - t0);
                if constexpr (kFilter) {
                    if (!(allowed[j >> 5] >> (j & 31) & 1u)) continue;
                }
                const double frac = (tf * k1p1) / (tf + st.norm[doc]);
                acc[j] = acc[j] + (w * frac);
                atomicOr(&touched[j >> 5], 1u << (j & 31));
                ++scored;
            }
        }
        __syncthreads();
    }
    if (scored) atomicAdd(s_scored, scored);

    // ---- 4: the touched documents that sort before the query's k-th kept entry go to its candidate list
    const uint64_t thr_key = ls.best_key[(int64_t)q * ls.k + ls.k - 1];
    const int32_t thr_doc = ls.best_doc[(int64_t)q * ls.k + ls.k - 1];
    for (int j = tid; j < T; j += kSparseThreads) {
        if (!(touched[j >> 5] >> (j & 31) & 1u)) continue;
        const uint64_t key = dist_to_key(-acc[j]);
        const int32_t doc = (int32_t)(t0 + j);
        if (!sparse_before(key, doc, thr_key, thr_doc)) continue;
        const unsigned slot = atomicAdd(&ls.count[q], 1u);
        if (slot < (unsigned)ls.cap) {
            ls.cand_key[(int64_t)q * ls.cap + slot] = key;
            ls.cand_doc[(int64_t)q * ls.cap + slot] = doc;
        }
    }
    __syncthreads();
    if (tid == 0 && *s_scored) atomicAdd(postings_scored, (unsigned long long)*s_scored);
}

constexpr int kSparsePairTerms = kSparseThreads;  // terms whose slice bounds one round stages in LDS, one per thread

struct SparsePairs {
    const int32_t* ids;  // local documents, -1: skipped.  row_stride = 0: [m], one list for every query; else [queries, row_stride]
    int64_t m;           // pairs per query
    int64_t row_stride;
    double* out_dist;    // [queries, m]: -score, NaN where skipped or unmatched.  null: the matches go to the candidate lists
    int q0;              // query blockIdx.y + q0 of the block
    int overlay;         // the layout has moved documents: `ov` is read
};

// grid: (ceil(m / kSparseThreads), queries of the launch), one thread per (query, listed document).  The document is looked
// up by binary search in the slice of each of the query's terms, ASCENDING: the base's slice while its `moved` bit is clear,
// the overlay's when it is set.  The operations and their order are k_sparse_score's, so the bits are too.  The chain of a
// thread is one dependent load per halving of a slice and nothing else: the slice bounds and weights of kSparsePairTerms
// terms at a time are staged in LDS by the block (they are the same for its threads), 10 KiB and few registers, so eight
// waves per SIMD hide each other's loads.  With lists, every match is appended: the caller keeps m <= ls.cap.
__global__ __launch_bounds__(kSparseThreads) void k_sparse_pairs(SparseStoreView st, SparseOverlayView ov, SparseQueries qs,
                                                                 SparseLists ls, SparsePairs pr, double k1p1,
                                                                 unsigned long long* __restrict__ postings_scored) {
    __shared__ int64_t s_p0[2][kSparsePairTerms], s_p1[2][kSparsePairTerms];
    __shared__ double s_w[kSparsePairTerms];
    __shared__ unsigned s_scored;
    const int tid = threadIdx.x;
    const int q = pr.q0 + (int)blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * kSparseThreads + tid;
    const int qo = qs.offsets[q];
    const int nt = qs.offsets[q + 1] - qo;  // (block-uniform)
    const int64_t d = j < pr.m ? (int64_t)pr.ids[(int64_t)blockIdx.y * pr.row_stride + j] : -1;
    int in_ov = 0;
    if (d >= 0 && pr.overlay && (d >> 5) < ov.moved_words) in_ov = (int)(ov.moved[d >> 5] >> (d & 31) & 1u);
    const int32_t* __restrict__ post_doc = in_ov ? ov.post_doc : st.post_doc;
    const uint16_t* __restrict__ post_tf = in_ov ? ov.post_tf : st.post_tf;
    const double norm = d >= 0 ? st.norm[d] : 0.0;
    if (tid == 0) s_scored = 0u;

    double score = 0.0;
    bool hit = false;
    unsigned scored = 0;
    for (int i0 = 0; i0 < nt; i0 += kSparsePairTerms) {
        const int ni = nt - i0 < kSparsePairTerms ? nt - i0 : kSparsePairTerms;
        __syncthreads();  // (the round before has been read)
        if (tid < ni) {
            const int t = qs.terms[qo + i0 + tid];
            s_w[tid] = qs.weights[qo + i0 + tid];
            const bool in_base = t >= 0 && t < st.vocab, in_over = pr.overlay && t >= 0 && t < ov.vocab;
            s_p0[0][tid] = in_base ? st.term_off[t] : 0;
            s_p1[0][tid] = in_base ? st.term_off[t + 1] : 0;
            s_p0[1][tid] = in_over ? ov.term_off[t] : 0;
            s_p1[1][tid] = in_over ? ov.term_off[t + 1] : 0;
        }
        __syncthreads();
        for (int i = 0; d >= 0 && i < ni; ++i) {
            const int64_t p0 = s_p0[in_ov][i], p1 = s_p1[in_ov][i];
            if (p0 == p1) continue;
            const int64_t p = sparse_lower_bound(post_doc, p0, p1, d);
            if (p == p1 || (int64_t)post_doc[p] != d) continue;
            const double tf = (double)post_tf[p];
            const double frac = (tf * k1p1) / (tf + norm);
            score = score + (s_w[i] * frac);
            hit = true;
            ++scored;
        }
    }
    if (pr.out_dist) {
        if (j < pr.m) pr.out_dist[(int64_t)blockIdx.y * pr.m + j] = hit ? -score : __longlong_as_double(0x7FF8000000000000ll);
    } else if (hit) {
        const unsigned slot = atomicAdd(&ls.count[q], 1u);
        if (slot < (unsigned)ls.cap) {
            ls.cand_key[(int64_t)q * ls.cap + slot] = dist_to_key(-score);
            ls.cand_doc[(int64_t)q * ls.cap + slot] = (int32_t)d;
        }
    }
    __syncthreads();  // (s_scored is zero for everyone, also when the query has no term)
    if (scored) atomicAdd(&s_scored, scored);
    __syncthreads();
    if (tid == 0 && s_scored) atomicAdd(postings_scored, (unsigned long long)s_scored);
}

__device__ __forceinline__ void bitonic_asc_sparse(uint64_t* key, int32_t* row, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int p = i ^ j;
                if (p > i) {
                    const bool asc = ((i & k) == 0);
                    const uint64_t ka = key[i], kb = key[p];
                    const int32_t ra = row[i], rb = row[p];
                    if (asc ? sparse_before(kb, rb, ka, ra) : sparse_before(ka, ra, kb, rb)) {
                        key[i] = kb;
                        key[p] = ka;
                        row[i] = rb;
                        row[p] = ra;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// grid: one workgroup per query of the launch.  np_max: the power of two >= k + cap the LDS was sized for.  flags: [nb] of the
// launch's chunk; a list that overflowed is dropped whole and flagged.
__global__ __launch_bounds__(kSparseThreads) void k_sparse_merge(SparseLists ls, const int* __restrict__ qlist, int np_max,
                                                                 int* __restrict__ flags) {
    extern __shared__ __align__(16) unsigned char sparse_smem[];
    uint64_t* key = (uint64_t*)sparse_smem;
    int32_t* row = (int32_t*)(key + np_max);
    const int tid = threadIdx.x;
    const int q = qlist ? qlist[blockIdx.x] : (int)blockIdx.x;
    const unsigned c = ls.count[q];  // (block-uniform: nobody writes it before the barrier below)
    __syncthreads();
    if (c == 0) return;
    if (tid == 0) ls.count[q] = 0;
    if (c > (unsigned)ls.cap) {
        if (tid == 0) flags[q] = 1;
        return;
    }
    const int n = ls.k + (int)c;
    const int np = next_pow2(n);  // <= np_max
    for (int i = tid; i < np; i += kSparseThreads) {
        uint64_t kk = kKeyNaN;
        int32_t rr = kRowNone;
        if (i < ls.k) {
            kk = ls.best_key[(int64_t)q * ls.k + i];
            rr = ls.best_doc[(int64_t)q * ls.k + i];
        } else if (i < n) {
            kk = ls.cand_key[(int64_t)q * ls.cap + (i - ls.k)];
            rr = ls.cand_doc[(int64_t)q * ls.cap + (i - ls.k)];
        }
        key[i] = kk;
        row[i] = rr;
    }
    __syncthreads();
    bitonic_asc_sparse(key, row, np);
    for (int i = tid; i < ls.k; i += kSparseThreads) {
        ls.best_key[(int64_t)q * ls.k + i] = key[i];
        ls.best_doc[(int64_t)q * ls.k + i] = row[i];
    }
}

// kept lists at "nothing yet", counters and flags at zero: n_best = nb * k, n_q = nb, n_flags = chunks * nb
__global__ __launch_bounds__(kSparseThreads) void k_sparse_reset(uint64_t* __restrict__ best_key, int32_t* __restrict__ best_doc,
                                                                 int64_t n_best, unsigned* __restrict__ count, int64_t n_q,
                                                                 int* __restrict__ flags, int64_t n_flags) {
    const int64_t i = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
    if (i < n_best) {
        best_key[i] = kKeyNaN;
        best_doc[i] = kRowNone;
    }
    if (i < n_q) count[i] = 0u;
    if (i < n_flags) flags[i] = 0;
}

__global__ __launch_bounds__(kSparseThreads) void k_sparse_final(const uint64_t* __restrict__ best_key,
                                                                 const int32_t* __restrict__ best_doc, int64_t n, int64_t row_offset,
                                                                 double* __restrict__ out_dist, int64_t* __restrict__ out_rows) {
    const int64_t i = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t r = best_doc[i];
    const bool has = r != kRowNone;
    out_dist[i] = has ? key_to_dist(best_key[i]) : __longlong_as_double(0x7FF8000000000000ll);
    out_rows[i] = has ? (int64_t)r + row_offset : -1;
}

}  // namespace mi355
