// subset_ids.h -- host side of a listed-subset call: the caller's GLOBAL row ids -> what k_scan_ids walks.
// Plain C++ (no HIP): a stand-alone program can include it and run it under a host sanitizer.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mi355 {

// a global row id as a local row of an index with `n` stored rows and option row_offset = `row_offset`; -1: not in this
// index (negative ids and -1 padding included) -- the rule of mi355dr_maxsim_subset
inline int64_t subset_local_row(int64_t global_id, int64_t row_offset, int64_t n) {
    // (ids and offsets are far apart at most by 2^63: the subtraction is done where it cannot wrap)
    if (global_id < row_offset) return -1;
    const uint64_t local = (uint64_t)global_id - (uint64_t)row_offset;
    return local < (uint64_t)n ? (int64_t)local : -1;
}

// ids[0 .. m) -> the local rows among them, ascending, each once (n < 2^31: they fit int32).  May throw std::bad_alloc.
inline void subset_prepare_ids(const int64_t* ids, int64_t m, int64_t row_offset, int64_t n, std::vector<int32_t>& out) {
    out.clear();
    out.reserve((size_t)std::min<int64_t>(m, n));
    bool sorted = true;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = subset_local_row(ids[i], row_offset, n);
        if (r < 0) continue;
        if (!out.empty() && (int32_t)r <= out.back()) sorted = false;
        if (out.size() == out.capacity()) out.reserve(out.capacity() * 2 + 16);  // (a list with many duplicates may exceed n)
        out.push_back((int32_t)r);
    }
    if (!sorted) {
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
    }
}

}  // namespace mi355
