// Stand-alone check of hgx_diff_wire's host plan (babble_amd/csrc/hgx_diff_host.cpp, no HIP): 400
// seeded random (known, last_index, chain_len, sync_limit) cases against a direct restatement of
// Core.OverSyncLimit / Core.Diff (node/core.go:147-188) over RollingIndex.Get
// (common/rolling_index.go:21-39), which here materialises every chain's item list. Meant for the
// host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibabble_amd/csrc \
//       tools/diff_host_check.cpp babble_amd/csrc/hgx_diff_host.cpp -o diff_host_check && ./diff_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "hgx_diff.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);       \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

// RollingIndex with its items spelled out (the Index of every cached event)
struct Rolling {
    int lastIndex = -1;
    std::vector<int> items;
    // Get(skipIndex): false = NewStoreErr(TooLate, string(SkippedIndex))
    bool get(int skipIndex, std::vector<int>& res) const {
        res.clear();
        if (skipIndex > lastIndex) return true;
        const int cachedItems = (int)items.size();
        const int oldestCachedIndex = lastIndex - cachedItems + 1;
        if (skipIndex + 1 < oldestCachedIndex) return false;
        const int start = skipIndex - oldestCachedIndex + 1;
        res.assign(items.begin() + start, items.end());
        return true;
    }
};

int main() {
    std::mt19937_64 rng(414);
    int64_t n_over = 0, n_late = 0, n_rows = 0, n_two = 0;
    for (int it = 0; it < 400; it++) {
        const int n = 1 + (int)(rng() % (it % 7 == 0 ? 1024 : 12));
        std::vector<Rolling> chains((size_t)n);
        std::vector<int32_t> known((size_t)n), last((size_t)n), len((size_t)n);
        for (int i = 0; i < n; i++) {
            Rolling& r = chains[(size_t)i];
            const int items = rng() % 5 == 0 ? 0 : (int)(rng() % 40);
            const int first = rng() % 3 == 0 ? (int)(rng() % 30) : 0;   // a pruned chain starts above 0
            if (items == 0) {
                r.lastIndex = rng() % 2 ? -1 : first - 1;   // no event yet: genesis, or a root's Index
            } else {
                for (int k = 0; k < items; k++) r.items.push_back(first + k);
                r.lastIndex = first + items - 1;
            }
            last[(size_t)i] = r.lastIndex;
            len[(size_t)i] = items;
            // around the window's edges: mostly inside, sometimes one or two below the oldest, or above the last
            const int oldest = r.lastIndex - items + 1;
            const uint64_t w = rng() % 16;
            known[(size_t)i] = w == 0 ? oldest - 2 - (int)(rng() % 3) : w == 1 ? oldest - 1 : w == 2 ? r.lastIndex + 1 + (int)(rng() % 4)
                                       : w == 3 ? r.lastIndex : oldest - 1 + (int)(rng() % (uint64_t)(items + 1));
        }
        // OverSyncLimit
        int64_t totUnknown = 0;
        for (int i = 0; i < n; i++)
            if (last[(size_t)i] > known[(size_t)i]) totUnknown += last[(size_t)i] - known[(size_t)i];
        const uint64_t lw = rng() % 6;
        const int64_t limit = lw == 0 ? -1 : lw == 1 ? totUnknown : lw == 2 ? totUnknown - 1 : lw == 3 ? 0 : (int64_t)(rng() % 400);
        const bool over = limit >= 0 && totUnknown > limit;
        // Diff, participants in ascending id
        int fail = -1, fails = 0;
        std::vector<int64_t> cnt((size_t)n, 0);
        int64_t total = 0;
        std::vector<int> res;
        for (int i = 0; i < n; i++) {
            if (!chains[(size_t)i].get(known[(size_t)i], res)) {
                if (fail < 0) fail = i;
                fails++;
                continue;
            }
            for (int idx : res) CHECK(idx > known[(size_t)i]);
            cnt[(size_t)i] = (int64_t)res.size();
            total += (int64_t)res.size();
        }
        hgx::DiffPlan p;
        hgx::diff_plan(known.data(), last.data(), len.data(), n, limit, p);
        CHECK(p.unknown == totUnknown);
        CHECK(p.over_limit == over);
        CHECK((int)p.count.size() == n);
        if (over) {
            CHECK(p.fail == -1 && p.total == 0 && p.msg.empty());
            n_over++;
            continue;
        }
        CHECK(p.fail == fail);
        if (fail >= 0) {
            CHECK(p.msg == std::string("\x03, Too Late") && p.total == 0);
            n_late++;
            n_two += fails > 1;
            continue;
        }
        CHECK(p.msg.empty() && p.total == total);
        for (int i = 0; i < n; i++) CHECK(p.count[(size_t)i] == cnt[(size_t)i]);
        n_rows += total;
    }
    // no participants at all
    hgx::DiffPlan p;
    hgx::diff_plan(nullptr, nullptr, nullptr, 0, 0, p);
    CHECK(!p.over_limit && p.fail == -1 && p.total == 0 && p.count.empty());
    CHECK(n_over > 20 && n_late > 20 && n_two > 5 && n_rows > 1000);
    std::printf("diff_host_check: 400 cases ok (%lld over the limit, %lld too late, %lld with two failing chains, %lld rows)\n",
                (long long)n_over, (long long)n_late, (long long)n_two, (long long)n_rows);
    return 0;
}
