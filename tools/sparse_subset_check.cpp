// sparse_subset_check.cpp -- csrc/sparse_subset.h (and subset_ids.h in front of it) exercised on the CPU, for a host sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iautorag_research_amd/csrc \
//       tools/sparse_subset_check.cpp -o sparse_subset_check && ./sparse_subset_check
// No HIP, no GPU: the headers are plain C++.  Every list -- random ones with duplicates, -1 padding and out-of-range ids,
// the tile-edge documents, m = 0 and m = n -- is turned into the bitmap, the launches with their tile lists and the pieces,
// and compared against a brute-force loop.  Exit status 0 and "sparse_subset_check ok" when every check holds.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <set>

#include "sparse_subset.h"
#include "subset_ids.h"

using namespace mi355;

#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

// one launch against the brute force: its documents are positions [p0, p1) of the list, its tiles those that hold one
static int check_launch(const SparseLaunch& l, const SparseLaunchPlan& plan, const std::vector<int32_t>& docs, int64_t p0, int64_t p1,
                        int T) {
    REQUIRE(p0 < p1 && p1 <= (int64_t)docs.size());
    REQUIRE(l.a0 == docs[(size_t)p0] && l.a1 == (int64_t)docs[(size_t)p1 - 1] + 1);
    int64_t inside = 0;
    for (const int32_t d : docs) inside += d >= l.a0 && d < l.a1;
    REQUIRE(inside == p1 - p0);  // the range holds the launch's listed documents and no other listed one
    std::set<int32_t> want;
    for (int64_t p = p0; p < p1; ++p) want.insert(docs[(size_t)p] / T);
    REQUIRE(l.n_tiles == (int)want.size() && l.tile_at >= 0 && l.tile_at + l.n_tiles <= (int64_t)plan.tiles.size());
    int i = 0;
    for (const int32_t t : want) REQUIRE(plan.tiles[(size_t)l.tile_at + i++] == t);  // ascending, each once
    return 0;
}

// brute force: which local documents are listed
static std::vector<char> brute_listed(const std::vector<int64_t>& ids, int64_t row_offset, int64_t n) {
    std::vector<char> listed((size_t)n, 0);
    for (const int64_t g : ids)
        for (int64_t d = 0; d < n; ++d)
            if (g == d + row_offset) listed[(size_t)d] = 1;
    return listed;
}

static int check_list(const std::vector<int64_t>& ids, const std::vector<char>& listed, int64_t row_offset, int64_t n, int k, int cap,
                      int T) {
    std::vector<int32_t> docs;
    subset_prepare_ids(ids.data(), (int64_t)ids.size(), row_offset, n, docs);
    size_t at = 0;
    for (int64_t d = 0; d < n; ++d)
        if (listed[(size_t)d]) REQUIRE(at < docs.size() && docs[at++] == d);
    REQUIRE(at == docs.size());

    // the one-pass form of a long list: the same documents, and their bitmap
    std::vector<int32_t> docs_scan = {7, 7};  // (what the vectors held before does not matter)
    std::vector<unsigned> bits = {1u};
    sparse_subset_scan(ids.data(), (int64_t)ids.size(), row_offset, n, docs_scan, bits);
    REQUIRE(docs_scan == docs && (int64_t)bits.size() == (n + 31) / 32);
    for (int64_t d = 0; d < (int64_t)bits.size() * 32; ++d)
        REQUIRE((bits[(size_t)(d >> 5)] >> (d & 31) & 1u) == (unsigned)(d < n && listed[(size_t)d]));

    const SparseLaunchPlan plan = sparse_plan_subset(docs, k, cap, T);
    const int64_t m = (int64_t)docs.size();
    if (m == 0) {
        REQUIRE(plan.ranges.empty() && plan.pieces.empty() && plan.tiles.empty());
        return 0;
    }
    const std::vector<int64_t> edges = sparse_plan(m, k, cap);
    REQUIRE(edges.front() == 0 && edges.back() == m && edges[1] <= cap);
    REQUIRE(plan.ranges.size() + 1 == edges.size() && plan.pieces.size() == plan.ranges.size() && plan.pieces[0].empty());
    for (size_t c = 0; c < plan.ranges.size(); ++c) {
        REQUIRE(edges[c] < edges[c + 1]);
        if (check_launch(plan.ranges[c], plan, docs, edges[c], edges[c + 1], T)) return 1;
        if (c == 0) continue;
        int64_t p = edges[c];  // the pieces: the range's positions in order, at most cap each, none left out
        for (const SparseLaunch& piece : plan.pieces[c]) {
            const int64_t p1 = std::min<int64_t>(p + cap, edges[c + 1]);
            if (check_launch(piece, plan, docs, p, p1, T)) return 1;
            p = p1;
        }
        REQUIRE(p == edges[c + 1]);
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20240607);
    const int64_t n = 1000;
    const int T = 256;
    // the plan over every document: ranges that tile [0, n), pieces of at most cap
    for (const int cap : {16, 64, 2048}) {
        const SparseLaunchPlan all = sparse_plan_all(n, 10, cap);
        int64_t at = 0;
        for (size_t c = 0; c < all.ranges.size(); ++c) {
            REQUIRE(all.ranges[c].a0 == at && all.ranges[c].n_tiles < 0);
            int64_t pa = at;
            for (const SparseLaunch& piece : all.pieces[c]) {
                REQUIRE(piece.a0 == pa && piece.a1 - piece.a0 <= cap && piece.n_tiles < 0);
                pa = piece.a1;
            }
            at = all.ranges[c].a1;
            REQUIRE(c == 0 ? all.pieces[c].empty() && at <= cap : pa == at);
        }
        REQUIRE(at == n);
    }
    REQUIRE(sparse_plan_all(0, 10, 16).ranges.empty());

    for (const int64_t row_offset : {(int64_t)0, (int64_t)10000, INT64_MIN + 3, INT64_MAX - 2000}) {
        std::vector<std::vector<int64_t>> lists;
        lists.push_back({});  // m = 0
        std::vector<int64_t> every;
        for (int64_t d = 0; d < n; ++d) every.push_back(d + row_offset);  // m = n
        lists.push_back(every);
        lists.push_back({row_offset, 255 + row_offset, 256 + row_offset, 511 + row_offset, 512 + row_offset, 767 + row_offset,
                         768 + row_offset, 999 + row_offset});  // tile edges
        lists.push_back({-1, -1, INT64_MIN, INT64_MAX, row_offset + n, row_offset + n - 1, row_offset + n - 1});
        for (int r = 0; r < 40; ++r) {  // random order, duplicates, padding, ids on both sides of the range
            std::vector<int64_t> l;
            const int len = (int)(rng() % 1500);
            const int64_t span = r % 4 == 0 ? 300 : n + 200;  // (every fourth list is confined to the first tiles)
            for (int i = 0; i < len; ++i) {
                const unsigned kind = (unsigned)(rng() % 10);
                // (the offset and the local part are added where the sum cannot overflow)
                const int64_t local = (int64_t)(rng() % (uint64_t)span) - 100;
                if (kind == 0) l.push_back(-1);
                else if (row_offset > 0 && local > INT64_MAX - row_offset) l.push_back(INT64_MAX);
                else if (row_offset < 0 && local < INT64_MIN - row_offset) l.push_back(INT64_MIN);
                else l.push_back(row_offset + local);
            }
            lists.push_back(l);
        }
        for (const auto& l : lists) {
            const std::vector<char> listed = brute_listed(l, row_offset, n);
            for (const int cap : {16, 64, 2048})
                for (const int k : {1, 10, 1024})
                    if (check_list(l, listed, row_offset, n, k, cap, T)) return 1;
        }
    }
    // a tile size above the store, and a store that ends on a tile edge
    const std::vector<int64_t> wide = {0, 5, 1023}, edge = {1023, 1024};
    if (check_list(wide, brute_listed(wide, 0, 1024), 0, 1024, 10, 16, 8192)) return 1;
    if (check_list(edge, brute_listed(edge, 0, 1024), 0, 1024, 10, 16, 256)) return 1;
    printf("sparse_subset_check ok\n");
    return 0;
}
