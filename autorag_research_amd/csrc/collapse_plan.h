// collapse_plan.h -- host side of mi355dr_search_collapsed*: the bookkeeping of the deepening schedule.
// Plain C++ (no HIP): a stand-alone program can include it and run it under a host sanitizer (tools/collapse_plan_check.cpp).
//
// A block of nb queries is searched at f = fetch_k and collapsed; k_collapse_lists leaves (kept, entries) per query.  A query is
// finished when it kept k, when its ranking ended (entries < f), or when f has reached max_fetch.  The others -- and only they
// -- are searched again at min(2 f, max_fetch).  The top-f list is a prefix of the top-2f list and the verdict on an entry
// depends on the entries before it alone, so the result is that of one pass at max_fetch whatever fetch_k was.
#pragma once
#include <stdint.h>

#include <vector>

namespace mi355 {

constexpr int kCollapseTruncated = 1;  // MI355DR_COLLAPSE_TRUNCATED

inline bool collapse_finished(int32_t kept, int32_t entries, int k, int f, int max_fetch) {
    return kept >= k || entries < f || f >= max_fetch;
}

// the width of the round behind one at f (f < max_fetch)
inline int collapse_next_fetch(int f, int max_fetch) { return (int)(2 * (int64_t)f < max_fetch ? 2 * (int64_t)f : max_fetch); }

// the state word and the line count of a finished query: truncated iff fewer than k were kept although the ranking was cut
inline int32_t collapse_state(int32_t kept, int32_t entries, int k, int max_fetch) {
    return kept < k && entries >= max_fetch ? kCollapseTruncated : 0;
}
inline int32_t collapse_count(int32_t kept, int k) { return kept < k ? kept : k; }

// One block's schedule.  `lines` holds the unfinished queries of the round that was just read back, ascending: list s of the
// next round belongs to query lines[s] (k_collapse_lists' slot-to-line list, k_gather_queries' map).
struct CollapsePlan {
    int nb = 0, k = 0, max_fetch = 0;
    int f = 0;                   // the width of the last round searched
    int64_t researched = 0;      // (query, round) re-searches so far
    std::vector<int32_t> lines;  // the queries of the NEXT round

    // before the first round: every query at fetch_k.  May throw std::bad_alloc (as may advance()).
    void begin(int nb_, int k_, int fetch_k, int max_fetch_) {
        nb = nb_;
        k = k_;
        max_fetch = max_fetch_;
        f = fetch_k;
        researched = 0;
        lines.resize((size_t)nb);
        for (int i = 0; i < nb; ++i) lines[(size_t)i] = i;
    }
    // kept / entries: [nb], by query, as read back after the round at f over `lines`.  Keeps the unfinished ones of them; when
    // any is left, f becomes the next round's width and true is returned.
    bool advance(const int32_t* kept, const int32_t* entries) {
        size_t n = 0;
        for (size_t s = 0; s < lines.size(); ++s) {
            const int32_t q = lines[s];
            if (!collapse_finished(kept[q], entries[q], k, f, max_fetch)) lines[n++] = q;
        }
        lines.resize(n);
        if (n == 0) return false;
        f = collapse_next_fetch(f, max_fetch);
        researched += (int64_t)n;
        return true;
    }
};

}  // namespace mi355
