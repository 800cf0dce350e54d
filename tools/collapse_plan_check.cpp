// collapse_plan_check.cpp -- csrc/collapse_plan.h exercised on the CPU, for a host sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iautorag_research_amd/csrc \
//       tools/collapse_plan_check.cpp -o collapse_plan_check && ./collapse_plan_check
// No HIP, no GPU: the header is plain C++.  Exit status 0 and "collapse_plan_check ok" when every check holds.
//
// The device side is played by a walk over synthetic rankings: query q's ranking is a list of keys (-1: no key), and a round
// at width f "searches" it by cutting it to f entries and counting (kept, entries) as k_collapse_lists does.  Every block
// is run through CollapsePlan and held against the walk at max_fetch, query by query.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "collapse_plan.h"

using namespace mi355;

#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

namespace {
using Ranking = std::vector<int64_t>;

// the walk over the first f entries: kept entries of the whole cut, and its entries
void walk(const Ranking& r, int f, int cap, int32_t* kept, int32_t* entries) {
    std::map<int64_t, int> seen;
    const int n = (int)r.size() < f ? (int)r.size() : f;
    int k = 0;
    for (int i = 0; i < n; ++i)
        if (r[(size_t)i] < 0 || seen[r[(size_t)i]]++ < cap) ++k;
    *kept = k;
    *entries = n;
}

// a ranking of `len` entries whose first `heavy` share one key, all others distinct
Ranking make(int len, int heavy) {
    Ranking r((size_t)len);
    for (int i = 0; i < len; ++i) r[(size_t)i] = i < heavy ? 7 : 1000 + i;
    return r;
}

// one block through the plan; 0 when it matches the walk at max_fetch and the independent count of re-searches
int run_block(const std::vector<Ranking>& block, int k, int cap, int fetch_k, int max_fetch) {
    const int nb = (int)block.size();
    std::vector<int32_t> kept((size_t)nb, -1), entries((size_t)nb, -1);
    std::vector<int> rounds((size_t)nb, 0);
    CollapsePlan plan;
    plan.begin(nb, k, fetch_k, max_fetch);
    REQUIRE((int)plan.lines.size() == nb && plan.f == fetch_k);
    for (int guard = 0;; ++guard) {
        REQUIRE(guard <= 12);  // fetch_k >= 1 doubles to 1024 in ten rounds
        REQUIRE(plan.f >= fetch_k && plan.f <= max_fetch);
        for (size_t s = 0; s < plan.lines.size(); ++s) {  // the round: only the plan's lines are written
            const int32_t q = plan.lines[s];
            REQUIRE(q >= 0 && q < nb && (s == 0 || plan.lines[s - 1] < q));
            walk(block[(size_t)q], plan.f, cap, &kept[(size_t)q], &entries[(size_t)q]);
            rounds[(size_t)q]++;
        }
        const int f_before = plan.f;
        const size_t n_before = plan.lines.size();
        if (!plan.advance(kept.data(), entries.data())) {
            REQUIRE(plan.lines.empty() && plan.f == f_before);
            break;
        }
        REQUIRE(!plan.lines.empty() && plan.lines.size() <= n_before);
        REQUIRE(f_before < max_fetch && plan.f == (2 * f_before < max_fetch ? 2 * f_before : max_fetch));
    }
    int64_t researched = 0;
    for (int q = 0; q < nb; ++q) {
        int32_t want_kept = 0, want_entries = 0;
        walk(block[(size_t)q], max_fetch, cap, &want_kept, &want_entries);
        // what the caller is given: the count and the state agree with one pass at max_fetch
        REQUIRE(collapse_count(kept[(size_t)q], k) == collapse_count(want_kept, k));
        REQUIRE(collapse_state(kept[(size_t)q], entries[(size_t)q], k, max_fetch) ==
                ((want_kept < k && want_entries == max_fetch) ? kCollapseTruncated : 0));
        // the rounds a query ran, counted on its own: widths fetch_k, 2 fetch_k, ... until it is finished
        int expect = 0;
        for (int f = fetch_k;; f = collapse_next_fetch(f, max_fetch)) {
            ++expect;
            int32_t a = 0, b = 0;
            walk(block[(size_t)q], f, cap, &a, &b);
            if (collapse_finished(a, b, k, f, max_fetch)) break;
        }
        REQUIRE(rounds[(size_t)q] == expect);
        researched += expect - 1;
    }
    REQUIRE(plan.researched == researched);
    return 0;
}
}  // namespace

int main() {
    // ---- the rules, one by one
    REQUIRE(collapse_finished(10, 16, 10, 16, 1024));    // kept k
    REQUIRE(collapse_finished(3, 15, 10, 16, 1024));     // the ranking ended
    REQUIRE(collapse_finished(3, 1024, 10, 1024, 1024)); // the last width
    REQUIRE(!collapse_finished(9, 16, 10, 16, 1024));
    REQUIRE(collapse_next_fetch(16, 1024) == 32 && collapse_next_fetch(512, 1024) == 1024 && collapse_next_fetch(256, 300) == 300 &&
            collapse_next_fetch(150, 300) == 300 && collapse_next_fetch(149, 300) == 298);
    REQUIRE(collapse_next_fetch(0x7FFFFFF0, 0x7FFFFFFF) == 0x7FFFFFFF);  // (no overflow in 2 f)
    REQUIRE(collapse_state(1, 1024, 2, 1024) == kCollapseTruncated && collapse_state(2, 1024, 2, 1024) == 0 &&
            collapse_state(1, 1023, 2, 1024) == 0 && collapse_state(0, 0, 2, 1024) == 0);
    REQUIRE(collapse_count(12, 10) == 10 && collapse_count(3, 10) == 3 && collapse_count(0, 10) == 0);

    // ---- B = 0: nothing to search, nothing to re-search
    {
        CollapsePlan plan;
        plan.begin(0, 10, 16, 1024);
        REQUIRE(plan.lines.empty() && !plan.advance(nullptr, nullptr) && plan.researched == 0 && plan.f == 16);
    }

    // ---- every unfinished-query pattern of a block of 4: each query is either light (finished in the first round) or one
    // of three heavy kinds (finished at a later width, truncated at max_fetch, ended early); all 4^4 blocks, at a power-of-two
    // and a non-power-of-two max_fetch, and with fetch_k == max_fetch (one round whatever the block holds)
    const int k = 10, cap = 1;
    for (const int max_fetch : {1024, 300}) {
        const Ranking kinds[4] = {make(2000, 1), make(2000, 120), make(2000, 1500), make(40, 35)};
        for (const int fetch_k : {10, 16, max_fetch}) {
            for (int code = 0; code < 256; ++code) {
                std::vector<Ranking> block;
                for (int q = 0, c = code; q < 4; ++q, c >>= 2) block.push_back(kinds[c & 3]);
                if (run_block(block, k, cap, fetch_k, max_fetch)) return 1;
            }
        }
        // fetch_k == max_fetch: no query is ever searched twice
        CollapsePlan once;
        once.begin(3, k, max_fetch, max_fetch);
        const int32_t kept[3] = {0, 5, 10}, entries[3] = {max_fetch, max_fetch, max_fetch};
        REQUIRE(!once.advance(kept, entries) && once.researched == 0);
    }
    // ---- caps above one, entries without a key, a full block of 1024 queries with every query unfinished at first
    for (const int c : {1, 2, 3}) {
        std::vector<Ranking> block;
        for (int q = 0; q < 1024; ++q) {
            Ranking r = make(1100, 20 + q % 400);
            if (q % 5 == 0)
                for (size_t i = 0; i < r.size(); i += 3) r[i] = -1;  // no key: never capped
            block.push_back(r);
        }
        if (run_block(block, 12, c, 12, 1000)) return 1;
    }
    printf("collapse_plan_check ok\n");
    return 0;
}
