// sparse_subset.h -- host side of a sparse search within a listed subset ("Within a listed subset"):
// the launch plan of a sparse search, and what the filtered tile pass needs of a sorted unique list of local documents --
// the bitmap, each launch's document range and the tiles that hold a listed document, the pieces of an overflowed launch.
// Plain C++ (no HIP): tools/sparse_subset_check.cpp includes it and runs it under a host sanitizer.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "subset_ids.h"

namespace mi355 {

// the launch plan of one block over n units (documents; listed documents of a subset): ranges [e, e') of growing size.  The
// first holds at most `cap` units, so its lists cannot overflow; after `seen` units a random order lets about
// k * new / seen of the next `new` beat the k-th kept entry, and the ratio keeps that at half a list.
inline std::vector<int64_t> sparse_plan(int64_t n, int k, int cap) {
    std::vector<int64_t> edges{0};
    const int64_t ratio = std::min<int64_t>(16, std::max<int64_t>(1, cap / (2 * (int64_t)k)));
    int64_t seen = std::min<int64_t>(n, cap);
    edges.push_back(seen);
    while (seen < n) {
        seen = std::min(n, seen + seen * ratio);
        edges.push_back(seen);
    }
    return edges;
}

// one launch of k_sparse_score: documents [a0, a1).  n_tiles < 0: every tile of the range (the unrestricted search); else
// the launch's tiles are tiles[tile_at .. tile_at + n_tiles) of the plan's tile array, ascending
struct SparseLaunch {
    int64_t a0, a1;
    int64_t tile_at;
    int n_tiles;
};

// what a search runs, launch by launch: pieces[c] are range c run again in parts that cannot overflow (none for c = 0)
struct SparseLaunchPlan {
    std::vector<SparseLaunch> ranges;
    std::vector<std::vector<SparseLaunch>> pieces;
    std::vector<int32_t> tiles;  // (a subset's plan only)
};

// every document of [0, n): sparse_plan over documents, pieces of at most `cap` documents
inline SparseLaunchPlan sparse_plan_all(int64_t n, int k, int cap) {
    SparseLaunchPlan p;
    if (n <= 0) return p;
    const std::vector<int64_t> edges = sparse_plan(n, k, cap);
    for (size_t c = 0; c + 1 < edges.size(); ++c) {
        p.ranges.push_back(SparseLaunch{edges[c], edges[c + 1], 0, -1});
        p.pieces.emplace_back();
        if (c == 0) continue;
        for (int64_t a = edges[c]; a < edges[c + 1]; a += cap)
            p.pieces.back().push_back(SparseLaunch{a, std::min<int64_t>(a + cap, edges[c + 1]), 0, -1});
    }
    return p;
}

// A long list from the caller's GLOBAL ids in one pass: the bitmap (one bit per document of [0, n): bit d & 31 of word d >> 5
// is set iff d is listed) and, read off its set bits in order, the listed local documents ascending, each once -- O(m + n / 32)
// where sorting the list first costs O(m log m) (a million scattered ids: 50 ms of the host's time against an 11 ms search).
// The rules are subset_prepare_ids': ids outside [row_offset, row_offset + n) are skipped, a value listed twice counts once.
// May throw std::bad_alloc.
inline void sparse_subset_scan(const int64_t* ids, int64_t m, int64_t row_offset, int64_t n, std::vector<int32_t>& docs,
                               std::vector<unsigned>& bits) {
    bits.assign((size_t)((n + 31) / 32), 0u);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t d = subset_local_row(ids[i], row_offset, n);
        if (d >= 0) bits[(size_t)(d >> 5)] |= 1u << (d & 31);
    }
    size_t count = 0;
    for (const unsigned w : bits) count += (size_t)__builtin_popcount(w);
    docs.clear();
    docs.reserve(count);
    for (size_t w = 0; w < bits.size(); ++w)
        for (unsigned rest = bits[w]; rest; rest &= rest - 1) docs.push_back((int32_t)(w * 32 + (size_t)__builtin_ctz(rest)));
}

// The listed documents docs[p0, p1) as one launch: the document range from the first to the last of them, and the tiles of T
// documents that hold one, appended to `tiles`.  The ranges of disjoint position ranges are disjoint, so a tile that two
// launches share is cut by each to its own documents.
inline SparseLaunch sparse_subset_launch(const std::vector<int32_t>& docs, int64_t p0, int64_t p1, int T, std::vector<int32_t>& tiles) {
    SparseLaunch l{(int64_t)docs[(size_t)p0], (int64_t)docs[(size_t)p1 - 1] + 1, (int64_t)tiles.size(), 0};
    for (int64_t p = p0; p < p1; ++p) {
        const int32_t t = docs[(size_t)p] / T;
        if (l.n_tiles == 0 || tiles.back() != t) {
            tiles.push_back(t);
            l.n_tiles++;
        }
    }
    return l;
}

// The plan in LISTED documents: sparse_plan over the positions of the list, mapped to document ranges; the first range holds
// at most `cap` listed documents, and the pieces of a later range at most `cap` each.  docs: ascending, distinct.
inline SparseLaunchPlan sparse_plan_subset(const std::vector<int32_t>& docs, int k, int cap, int T) {
    SparseLaunchPlan p;
    const int64_t m = (int64_t)docs.size();
    if (m == 0) return p;
    const std::vector<int64_t> edges = sparse_plan(m, k, cap);
    for (size_t c = 0; c + 1 < edges.size(); ++c) {
        p.ranges.push_back(sparse_subset_launch(docs, edges[c], edges[c + 1], T, p.tiles));
        p.pieces.emplace_back();
        if (c == 0) continue;
        for (int64_t a = edges[c]; a < edges[c + 1]; a += cap)
            p.pieces.back().push_back(sparse_subset_launch(docs, a, std::min<int64_t>(a + cap, edges[c + 1]), T, p.tiles));
    }
    return p;
}

}  // namespace mi355
