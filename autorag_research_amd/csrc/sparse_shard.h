// sparse_shard.h -- host side of the row-sharded sparse searches: the sorted union of a call's
// query terms, the layout of the statistics payload a rank contributes, and the split of the folded (summed) row back into
// per-query BM25 weights.  Every rank runs these over the same queries and the same folded integers, so every rank gets
// the same terms and calls log() on the same arguments.
// Plain C++ (no HIP): tools/sparse_shard_check.cpp includes it and runs it under a host sanitizer.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mi355 {

// the statistics payload of one rank, int64 [kShardStatsHead + T]: n_live, total_len, then df(t) of the call's terms
constexpr int kShardStatsHead = 2;

// The distinct terms of ALL queries of a BM25 call that lie inside [0, term_limit), ascending, each once: the terms whose df
// travels.  Query j is q_tokens[q_offsets[j] .. q_offsets[j + 1]) (q_offsets never decreases; raw tokens, repeats allowed).
// Returns the first query with more than terms_max DISTINCT tokens (in range or not: the local form's rule), else -1.
// May throw std::bad_alloc.
inline int shard_query_terms(const int32_t* q_tokens, const int32_t* q_offsets, int B, int32_t term_limit, int terms_max,
                             std::vector<int32_t>& terms) {
    terms.clear();
    std::vector<int32_t> one;
    for (int q = 0; q < B; ++q) {
        const int32_t lo = q_offsets[q], hi = q_offsets[q + 1];
        if (hi <= lo) continue;
        one.assign(q_tokens + lo, q_tokens + hi);
        std::sort(one.begin(), one.end());
        one.erase(std::unique(one.begin(), one.end()), one.end());
        if ((int64_t)one.size() > terms_max) return q;
        for (const int32_t t : one)
            if (t >= 0 && t < term_limit) terms.push_back(t);
    }
    std::sort(terms.begin(), terms.end());
    terms.erase(std::unique(terms.begin(), terms.end()), terms.end());
    return -1;
}

// This rank's payload: df_of(t) is the shard's document frequency of term t (0 for a term it has never seen).
template <class DfOf>
inline void shard_stats_payload(int64_t n_live, int64_t total_len, const std::vector<int32_t>& terms, DfOf df_of,
                                std::vector<int64_t>& payload) {
    payload.resize((size_t)kShardStatsHead + terms.size());
    payload[0] = n_live;
    payload[1] = total_len;
    for (size_t i = 0; i < terms.size(); ++i) payload[(size_t)kShardStatsHead + i] = df_of(terms[i]);
}

// the BM25 weight of a term with document frequency df among N documents (include/mi355dr.h, "sparse store")
inline double shard_bm25_weight(int64_t N, int64_t df) { return log(1.0 + (((double)(N - df) + 0.5) / ((double)df + 0.5))); }

// The folded row [kShardStatsHead + terms.size()] (the ranks' payloads summed) back into the call's queries as the weighted
// search takes them: per query its distinct in-range tokens with GLOBAL df > 0, ascending, weighted from the global N and df;
// offsets [B + 1].  `terms` is shard_query_terms' output for the same queries.  May throw std::bad_alloc.
inline void shard_split_weights(const int32_t* q_tokens, const int32_t* q_offsets, int B, const std::vector<int32_t>& terms,
                                const int64_t* folded, std::vector<int32_t>& out_terms, std::vector<double>& out_weights,
                                std::vector<int32_t>& out_offsets) {
    const int64_t N = folded[0];
    out_terms.clear();
    out_weights.clear();
    out_offsets.assign((size_t)B + 1, 0);
    std::vector<int32_t> one;
    for (int q = 0; q < B; ++q) {
        const int32_t lo = q_offsets[q], hi = q_offsets[q + 1];
        one.clear();
        if (hi > lo) one.assign(q_tokens + lo, q_tokens + hi);
        std::sort(one.begin(), one.end());
        one.erase(std::unique(one.begin(), one.end()), one.end());
        for (const int32_t t : one) {
            const auto it = std::lower_bound(terms.begin(), terms.end(), t);
            if (it == terms.end() || *it != t) continue;  // outside [0, term_limit)
            const int64_t df = folded[(size_t)kShardStatsHead + (size_t)(it - terms.begin())];
            if (df <= 0) continue;
            out_terms.push_back(t);
            out_weights.push_back(shard_bm25_weight(N, df));
        }
        out_offsets[(size_t)q + 1] = (int32_t)out_terms.size();
    }
}

}  // namespace mi355
