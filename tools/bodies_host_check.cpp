// Stand-alone check of the event-body front end's host side (babble_amd/csrc/hgx_bodies_host.cpp,
// no HIP): random batches through the argument checks, hgx_batch_levels, the cut, the chunk plan and
// the level plan, with the plans' invariants asserted. Meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibabble_amd/csrc \
//       tools/bodies_host_check.cpp babble_amd/csrc/hgx_bodies_host.cpp -o bodies_host_check && ./bodies_host_check
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hgx.h"
#include "hgx_bodies.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);       \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

int main() {
    std::mt19937_64 rng(2024);
    int64_t events = 0;
    for (int it = 0; it < 400; it++) {
        const int n = 1 + (int)(rng() % 9), graphs = 1 + (int)(rng() % 3);
        const int64_t count = (int64_t)(rng() % 700), base = (int64_t)(rng() % 50);
        std::vector<int32_t> creator((size_t)count), ntx((size_t)count);
        std::vector<int64_t> index((size_t)count), sp((size_t)count), op((size_t)count), ts((size_t)count), tx_off(1, 0);
        std::vector<uint8_t> r((size_t)count * 32 + 1), s((size_t)count * 32 + 1), bytes(1);
        for (int64_t k = 0; k < count; k++) {
            const int64_t g = base + k;
            creator[(size_t)k] = (int32_t)(rng() % (uint64_t)(n * graphs));
            sp[(size_t)k] = g == 0 || rng() % 5 == 0 ? -1 : (int64_t)(rng() % (uint64_t)g);
            op[(size_t)k] = g == 0 || rng() % 5 == 0 ? -1 : (int64_t)(rng() % (uint64_t)g);
            ntx[(size_t)k] = (int32_t)(rng() % 5) - 1;
            for (int j = 0; j < ntx[(size_t)k]; j++) {
                const size_t len = rng() % 3 == 0 ? 0 : rng() % 200;
                bytes.resize(bytes.size() + len, (uint8_t)it);
                tx_off.push_back((int64_t)bytes.size() - 1);
            }
        }
        const hgx::BodiesIn ev{creator.data(), index.data(), sp.data(), op.data(), ts.data(), r.data(), s.data(),
                               ntx.data(), tx_off.data(), bytes.data()};
        std::vector<int64_t> txi;
        CHECK(hgx::bodies_check(ev, count, txi) == nullptr);
        CHECK((int64_t)txi.size() == count + 1 && txi[(size_t)count] == (int64_t)tx_off.size() - 1);
        CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs) == count);
        // the C entry and the level rule
        std::vector<int32_t> level((size_t)count + 1, -7);
        int32_t nl = -1;
        hgx_error err;
        CHECK(hgx_batch_levels(sp.data(), op.data(), count, base, level.data(), &nl, &err) == HGX_OK);
        CHECK(level[(size_t)count] == -7);
        int32_t top = 0;
        for (int64_t k = 0; k < count; k++) {
            int32_t want = 0;
            if (sp[(size_t)k] >= base) want = level[(size_t)(sp[(size_t)k] - base)] + 1;
            if (op[(size_t)k] >= base && level[(size_t)(op[(size_t)k] - base)] + 1 > want) want = level[(size_t)(op[(size_t)k] - base)] + 1;
            CHECK(level[(size_t)k] == want);
            if (want + 1 > top) top = want + 1;
        }
        CHECK(nl == top);
        // the level plan: every position once, inside its own graph's workgroup, at its level
        hgx::LevelPlan plan;
        hgx::plan_levels(creator.data(), level.data(), count, n, plan);
        CHECK((int64_t)plan.pos.size() == count && plan.wg_lo.size() == plan.wg_nl.size());
        std::vector<int> seen((size_t)count, 0);
        int32_t widest = 0;
        for (size_t j = 0; j < plan.wg_lo.size(); j++) {
            int graph = -1;
            for (int32_t l = 0; l < plan.wg_nl[j]; l++) {
                const int32_t a = plan.loff[(size_t)(plan.wg_lo[j] + l)], b = plan.loff[(size_t)(plan.wg_lo[j] + l + 1)];
                CHECK(a <= b && b <= count);
                if (b - a > widest) widest = b - a;
                for (int32_t i = a; i < b; i++) {
                    const int32_t k = plan.pos[(size_t)i];
                    CHECK(k >= 0 && k < count && level[(size_t)k] == l);
                    if (graph < 0) graph = creator[(size_t)k] / n;
                    CHECK(creator[(size_t)k] / n == graph);
                    seen[(size_t)k]++;
                }
            }
        }
        for (int64_t k = 0; k < count; k++) CHECK(seen[(size_t)k] == 1);
        CHECK(widest == plan.max_width);
        // the chunk plan covers the batch in order
        for (int64_t lo = 0; lo < count;) {
            int64_t bound = 0;
            const int64_t hi = hgx::bodies_chunk_end(ev, txi, lo, count, &bound);
            CHECK(hi > lo && hi <= count && hi - lo <= hgx::kBodyChunkEvents && bound >= (hi - lo) * hgx::kBodyFixedBytes);
            lo = hi;
        }
        // rejected inputs
        if (count > 3) {
            const int64_t k = (int64_t)(rng() % (uint64_t)count);
            const int64_t keep = op[(size_t)k];
            op[(size_t)k] = base + k + (int64_t)(rng() % 2);
            CHECK(hgx_batch_levels(sp.data(), op.data(), count, base, level.data(), &nl, &err) == HGX_ERR_INVALID);
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs) == k);
            op[(size_t)k] = HGX_UNKNOWN_PARENT;
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs) == k);
            // the root codes have a text on a context with root ids only
            std::vector<uint8_t> has_y((size_t)(n * graphs), 0);
            op[(size_t)k] = HGX_ROOT_Y;
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs) == k);
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs, has_y.data(), true) == k);
            has_y[(size_t)creator[(size_t)k]] = 1;
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs, has_y.data(), false) == count);
            op[(size_t)k] = HGX_ROOT_OTHER;
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs, has_y.data(), false) == k);
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs, has_y.data(), true) == count);
            CHECK(hgx_batch_levels(sp.data(), op.data(), count, base, level.data(), &nl, &err) == HGX_OK);
            op[(size_t)k] = -5;
            CHECK(hgx::bodies_first_unencodable(ev, count, base, n * graphs, has_y.data(), true) == k);
            op[(size_t)k] = keep;
            if (tx_off.size() > 2) {
                tx_off[1] += 1000000000;
                CHECK(hgx::bodies_check(ev, count, txi) != nullptr);
                tx_off[1] -= 1000000000;
            }
            ntx[(size_t)k] = -2;
            CHECK(hgx::bodies_check(ev, count, txi) != nullptr);
        }
        events += count;
    }
    CHECK(hgx_batch_levels(nullptr, nullptr, 3, 0, nullptr, nullptr, nullptr) == HGX_ERR_INVALID);
    CHECK(hgx_batch_levels(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == HGX_OK);
    std::printf("bodies_host_check: 400 batches, %lld events, ok\n", (long long)events);
    return 0;
}
