// mmr_order_check.cpp -- csrc/mmr_order.h (and subset_ids.h under it) exercised on the CPU, for a host sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iautorag_research_amd/csrc \
//       tools/mmr_order_check.cpp -o mmr_order_check && ./mmr_order_check
// No HIP, no GPU: the header is plain C++.  Exit status 0 and "mmr_order_check ok" when every check holds.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "mmr_order.h"

using namespace mi355;

#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    // ---- keys: the device's dist_to_key order, -0 before +0, NaN last
    REQUIRE(mmr_dist_key(-1.0) < mmr_dist_key(-0.0));
    REQUIRE(mmr_dist_key(-0.0) < mmr_dist_key(0.0));
    REQUIRE(mmr_dist_key(0.0) < mmr_dist_key(1e-300));
    REQUIRE(mmr_dist_key(2.0) < mmr_dist_key(INFINITY));
    REQUIRE(mmr_dist_key(INFINITY) < mmr_dist_key(NAN));
    REQUIRE(mmr_dist_key(-INFINITY) < mmr_dist_key(-1e300));

    // ---- list hygiene: offsets, padding, out-of-range ids at both ends of int64, duplicates, appended lists
    const int64_t off = 1000, n = 50;
    const int64_t ids[] = {1049, 1000, -1, 999, 1050, 1007, 1007, INT64_MIN, INT64_MAX, 1049, 0, 1001};
    std::vector<int64_t> rows = {77};  // (an earlier query's rows stay in front, untouched)
    REQUIRE(mmr_unique_rows(ids, (int64_t)(sizeof(ids) / sizeof(ids[0])), off, n, rows) == 4);
    REQUIRE(rows.size() == 5 && rows[0] == 77 && rows[1] == 0 && rows[2] == 1 && rows[3] == 7 && rows[4] == 49);
    REQUIRE(mmr_unique_rows(ids, 0, off, n, rows) == 0 && rows.size() == 5);
    REQUIRE(mmr_unique_rows(nullptr, 0, off, n, rows) == 0);
    const int64_t low[] = {INT64_MIN + 5, INT64_MIN, INT64_MIN + 5, INT64_MAX, 0};  // extreme offset: the subtraction must not wrap
    REQUIRE(mmr_unique_rows(low, 5, INT64_MIN, 10, rows) == 2 && rows[5] == 0 && rows[6] == 5);

    // ---- the total order: distance asc, NaN last, row asc
    MmrCand list[] = {{0.5, 9}, {NAN, 2}, {0.5, 3}, {-0.0, 8}, {0.0, 1}, {NAN, 0}, {-2.0, 4}, {INFINITY, 5}};
    mmr_order(list, 8);
    const int64_t want[] = {4, 8, 1, 3, 9, 5, 0, 2};
    for (int i = 0; i < 8; ++i) REQUIRE(list[i].row == want[i]);
    mmr_order(list, 0);
    mmr_order(nullptr, 0);

    // ---- the cap: 1024 candidates with many ties and NaNs, against a sort of (key, row) pairs
    std::mt19937_64 rng(5);
    std::vector<MmrCand> big(1024);
    for (size_t i = 0; i < big.size(); ++i) {
        const int v = (int)(rng() % 37);
        big[i] = MmrCand{v == 0 ? (double)NAN : (v - 18) * 0.125, (int64_t)(rng() % 100000)};
    }
    mmr_order(big.data(), (int64_t)big.size());
    for (size_t i = 1; i < big.size(); ++i) {
        const uint64_t ka = mmr_dist_key(big[i - 1].dist), kb = mmr_dist_key(big[i].dist);
        REQUIRE(ka < kb || (ka == kb && big[i - 1].row <= big[i].row));
    }
    printf("mmr_order_check ok\n");
    return 0;
}
