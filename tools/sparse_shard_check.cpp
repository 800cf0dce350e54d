// sparse_shard_check.cpp -- csrc/sparse_shard.h exercised on the CPU, for a host sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iautorag_research_amd/csrc \
//       tools/sparse_shard_check.cpp -o sparse_shard_check && ./sparse_shard_check
// No HIP, no GPU: the header is plain C++.  The sorted union of a call's query terms, the statistics payload and the split of
// the folded row into per-query weights are run over the edge inputs -- no query, queries without a term, every term out of
// range, 1024- and 1025-term queries, repeated tokens -- and over random calls against a brute-force loop: shards' payloads
// summed by hand must give the weights one store holding every document computes.  Exit status 0 and
// "sparse_shard_check ok" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <set>

#include "sparse_shard.h"

using namespace mi355;

#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

constexpr int32_t kLimit = 1 << 20;
constexpr int kTermsMax = 1024;

struct Queries {
    std::vector<int32_t> tokens, offsets{0};
    void add(const std::vector<int32_t>& q) {
        tokens.insert(tokens.end(), q.begin(), q.end());
        offsets.push_back((int32_t)tokens.size());
    }
    int B() const { return (int)offsets.size() - 1; }
};

// one call over `world` shards with the given df tables: union, payloads, fold by hand, split; checked against a brute force
static int check_call(const Queries& qs, const std::vector<std::map<int32_t, int64_t>>& df, const std::vector<int64_t>& n_live,
                      const std::vector<int64_t>& total_len) {
    const int B = qs.B();
    std::vector<int32_t> uni = {5, 5, 1};  // (what the vector held before does not matter)
    const int bad = shard_query_terms(qs.tokens.data(), qs.offsets.data(), B, kLimit, kTermsMax, uni);
    // brute force: the set of in-range tokens, and the first query with too many distinct ones
    std::set<int32_t> want;
    int want_bad = -1;
    for (int q = 0; q < B && want_bad < 0; ++q) {
        std::set<int32_t> one(qs.tokens.begin() + qs.offsets[q], qs.tokens.begin() + qs.offsets[q + 1]);
        if ((int)one.size() > kTermsMax) want_bad = q;
        else
            for (const int32_t t : one)
                if (t >= 0 && t < kLimit) want.insert(t);
    }
    REQUIRE(bad == want_bad);
    if (bad >= 0) return 0;
    REQUIRE(std::vector<int32_t>(want.begin(), want.end()) == uni);

    std::vector<int64_t> folded((size_t)kShardStatsHead + uni.size(), 0), payload = {9};
    for (size_t r = 0; r < df.size(); ++r) {
        shard_stats_payload(n_live[r], total_len[r], uni,
                            [&](int32_t t) -> int64_t {
                                const auto it = df[r].find(t);
                                return it == df[r].end() ? 0 : it->second;
                            },
                            payload);
        REQUIRE(payload.size() == folded.size() && payload[0] == n_live[r] && payload[1] == total_len[r]);
        for (size_t i = 0; i < folded.size(); ++i) folded[i] += payload[i];
    }
    std::vector<int32_t> terms = {3}, offsets = {1, 2};
    std::vector<double> weights = {1.0};
    shard_split_weights(qs.tokens.data(), qs.offsets.data(), B, uni, folded.data(), terms, weights, offsets);
    REQUIRE((int)offsets.size() == B + 1 && offsets[0] == 0 && terms.size() == weights.size());
    const int64_t N = folded[0];
    for (int q = 0; q < B; ++q) {
        std::set<int32_t> one(qs.tokens.begin() + qs.offsets[q], qs.tokens.begin() + qs.offsets[q + 1]);
        int32_t at = offsets[q];
        for (const int32_t t : one) {  // ascending
            if (t < 0 || t >= kLimit) continue;
            int64_t g = 0;
            for (const auto& shard : df) {
                const auto it = shard.find(t);
                if (it != shard.end()) g += it->second;
            }
            if (g == 0) continue;
            REQUIRE(at < offsets[q + 1] && terms[(size_t)at] == t);
            const double w = log(1.0 + (((double)(N - g) + 0.5) / ((double)g + 0.5)));
            REQUIRE(memcmp(&w, &weights[(size_t)at], sizeof(w)) == 0);
            ++at;
        }
        REQUIRE(at == offsets[q + 1] && offsets[q + 1] - offsets[q] <= kTermsMax);
    }
    REQUIRE(offsets[B] == (int32_t)terms.size());
    return 0;
}

int main() {
    std::mt19937_64 rng(20240911);
    const std::vector<std::map<int32_t, int64_t>> two = {{{1, 3}, {7, 1}, {kLimit - 1, 2}}, {{7, 4}, {9, 1}}};
    const std::vector<int64_t> live = {5, 6}, len = {40, 77};
    {  // no query (null pointers are never read: B = 0)
        std::vector<int32_t> uni, terms, offsets;
        std::vector<double> weights;
        const int32_t zero = 0;
        REQUIRE(shard_query_terms(nullptr, &zero, 0, kLimit, kTermsMax, uni) == -1 && uni.empty());
        const int64_t folded[2] = {11, 117};
        shard_split_weights(nullptr, &zero, 0, uni, folded, terms, weights, offsets);
        REQUIRE(terms.empty() && weights.empty() && offsets == std::vector<int32_t>{0});
    }
    {  // queries without a term, alone and between others
        Queries qs;
        qs.add({});
        if (check_call(qs, two, live, len)) return 1;
        qs.add({7, 7, 1});
        qs.add({});
        if (check_call(qs, two, live, len)) return 1;
    }
    {  // every term out of range; repeated tokens; a term no shard holds; the largest term id
        Queries qs;
        qs.add({-1, kLimit, INT32_MAX, INT32_MIN, -1});
        qs.add({7, 7, 7, 7});
        qs.add({8, 9, 8, 1, kLimit - 1, kLimit});
        if (check_call(qs, two, live, len)) return 1;
    }
    {  // 1024 distinct terms pass, with repeats on top; 1025 are refused, in range or not; shards without any document
        Queries qs;
        std::vector<int32_t> big;
        for (int i = 0; i < kTermsMax; ++i) big.push_back(3 * i);
        std::vector<int32_t> rep = big;
        rep.insert(rep.end(), big.begin(), big.end());
        qs.add(rep);
        std::vector<std::map<int32_t, int64_t>> many(3);
        for (int i = 0; i < kTermsMax; i += 2) many[(size_t)(i % 3)][3 * i] = 1 + i % 5;
        if (check_call(qs, many, {0, 900, 2000}, {0, 1, 123456789012ll})) return 1;
        if (check_call(qs, {{}, {}}, {0, 0}, {0, 0})) return 1;  // global N = 0: no term survives
        big.push_back(-5);
        Queries over;
        over.add({1});
        over.add(big);
        std::vector<int32_t> uni;
        REQUIRE(shard_query_terms(over.tokens.data(), over.offsets.data(), over.B(), kLimit, kTermsMax, uni) == 1);
        if (check_call(over, two, live, len)) return 1;
    }
    for (int r = 0; r < 200; ++r) {  // random calls over 1 .. 8 shards
        const int world = 1 + (int)(rng() % 8);
        std::vector<std::map<int32_t, int64_t>> df((size_t)world);
        std::vector<int64_t> n_live, total;
        for (int w = 0; w < world; ++w) {
            const int64_t n = (int64_t)(rng() % 1000);
            n_live.push_back(n);
            total.push_back(n * (int64_t)(rng() % 50));
            const int nt = n ? (int)(rng() % 60) : 0;
            for (int i = 0; i < nt; ++i) df[(size_t)w][(int32_t)(rng() % 80)] = 1 + (int64_t)(rng() % (uint64_t)n);
        }
        Queries qs;
        const int B = (int)(rng() % 12);
        for (int q = 0; q < B; ++q) {
            std::vector<int32_t> one;
            const int len_q = (int)(rng() % 20);
            for (int i = 0; i < len_q; ++i) one.push_back((int32_t)(rng() % 100) - 5);
            qs.add(one);
        }
        if (check_call(qs, df, n_live, total)) return 1;
    }
    printf("sparse_shard_check ok\n");
    return 0;
}
