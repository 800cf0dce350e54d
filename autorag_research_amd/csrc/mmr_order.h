// mmr_order.h -- host side of mi355dr_mmr_select: one query's candidate list -> the order k_mmr_select expects.
// Plain C++ (no HIP): a stand-alone program can include it and run it under a host sanitizer (tools/mmr_order_check.cpp).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "subset_ids.h"

namespace mi355 {

// host image of dist_to_key (dev_common.h): unsigned compare == (distance asc, -0 before +0, NaN last)
inline uint64_t mmr_dist_key(double d) {
    if (d != d) return 0xFFFFFFFFFFFFFFFFull;
    uint64_t b;
    memcpy(&b, &d, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct MmrCand {
    double dist;   // the query's exact distance to the row (NaN: removed row, undefined distance)
    int64_t row;   // local row
};

// ids[0 .. m) of ONE query -> the local rows among them, ascending, each once: the hygiene of mi355dr_search_subset
// (ids outside the index and -1 padding skipped).  Appends to `out`, returns how many.  May throw std::bad_alloc.
inline int64_t mmr_unique_rows(const int64_t* ids, int64_t m, int64_t row_offset, int64_t n, std::vector<int64_t>& out) {
    const size_t first = out.size();
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = subset_local_row(ids[i], row_offset, n);
        if (r >= 0) out.push_back(r);
    }
    std::sort(out.begin() + (ptrdiff_t)first, out.end());
    out.erase(std::unique(out.begin() + (ptrdiff_t)first, out.end()), out.end());
    return (int64_t)(out.size() - first);
}

// list[0 .. m) into the library's total order: distance asc, NaN last, row asc
inline void mmr_order(MmrCand* list, int64_t m) {
    std::sort(list, list + m, [](const MmrCand& a, const MmrCand& b) {
        const uint64_t ka = mmr_dist_key(a.dist), kb = mmr_dist_key(b.dist);
        return ka < kb || (ka == kb && a.row < b.row);
    });
}

}  // namespace mi355
