// Stand-alone check of the body store's host side (babble_amd/csrc/hgx_bodystore_host.cpp, no HIP):
//  - block_text_len against the length of the text a host encoder writes (Go's json.Encoder over
//    Block{RoundReceived, Transactions}, block.go:44-53: built here as a string, byte by byte) on 400
//    seeded random blocks, plus the edges (null, [], empty transactions, every length mod 3, negative
//    and 19-digit RoundReceived);
//  - block_text_bound (what hgx_find_order refuses by) never below that text, and the 4 GiB rule;
//  - body_grow_plan against a direct restatement (double until it fits) on seeded random pairs;
//  - the capacity rule and hgx_keep_bodies' argument check, case by case.
// Meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibabble_amd/csrc \
//       tools/bodystore_host_check.cpp babble_amd/csrc/hgx_bodystore_host.cpp -o bodystore_host_check && \
//       ./bodystore_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hgx_bodystore.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);       \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static void base64(const std::vector<uint8_t>& in, std::string& out) {
    static const char T[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    size_t i = 0;
    for (; i + 3 <= in.size(); i += 3) {
        const uint32_t v = (uint32_t)in[i] << 16 | (uint32_t)in[i + 1] << 8 | in[i + 2];
        out += T[v >> 18]; out += T[(v >> 12) & 63]; out += T[(v >> 6) & 63]; out += T[v & 63];
    }
    const size_t rem = in.size() - i;
    if (rem) {
        const uint32_t v = (uint32_t)in[i] << 16 | (rem == 2 ? (uint32_t)in[i + 1] << 8 : 0u);
        out += T[v >> 18]; out += T[(v >> 12) & 63];
        out += rem == 2 ? T[(v >> 6) & 63] : '=';
        out += '=';
    }
}

static std::string block_text(int64_t rr, const std::vector<std::vector<uint8_t>>& txs, bool nil) {
    std::string s = "{\"RoundReceived\":" + std::to_string(rr) + ",\"Transactions\":";
    if (nil && txs.empty()) {
        s += "null";
    } else {
        s += '[';
        for (size_t i = 0; i < txs.size(); i++) {
            if (i) s += ',';
            s += '"';
            base64(txs[i], s);
            s += '"';
        }
        s += ']';
    }
    return s + "}\n";
}

static void check_block(int64_t rr, const std::vector<std::vector<uint8_t>>& txs, bool nil) {
    std::vector<int64_t> off(txs.size() + 1, 0);
    for (size_t i = 0; i < txs.size(); i++) off[i + 1] = off[i] + (int64_t)txs[i].size();
    const int64_t want = (int64_t)block_text(rr, txs, nil).size();
    CHECK(hgx::block_text_len(rr, (int32_t)txs.size(), nil, off.data()) == want);
    // the bound hgx_find_order refuses by (it has the totals only) is never below the text
    CHECK(hgx::block_text_bound(1, (int64_t)txs.size(), off.back()) >= want);
}

static int64_t grow_restated(int64_t cap, int64_t need) {
    if (need <= cap) return cap;
    int64_t c = cap > hgx::kBodyMinCap ? cap : hgx::kBodyMinCap;
    while (c < need) c += c;
    return c;
}

int main() {
    std::mt19937_64 rng(20260601);
    auto bytes = [&](size_t len) {
        std::vector<uint8_t> v(len);
        for (auto& b : v) b = (uint8_t)rng();
        return v;
    };
    // the edges
    for (int64_t rr : {(int64_t)0, (int64_t)9, (int64_t)10, (int64_t)999, (int64_t)1000, (int64_t)123456, (int64_t)-1,
                       (int64_t)-10, INT64_MAX, INT64_MIN}) {
        check_block(rr, {}, true);
        check_block(rr, {}, false);
        for (size_t len = 0; len <= 200; len++) check_block(rr, {bytes(len)}, false);
    }
    check_block(7, std::vector<std::vector<uint8_t>>(1000), false);   // 1 000 empty transactions
    check_block(7, {bytes(200000)}, true);                            // (nil first event, transactions appended)
    int cases = 0;
    for (; cases < 400; cases++) {
        const int64_t rr = (int64_t)(rng() % 4 == 0 ? rng() >> (rng() % 64) : rng() % 100000);
        std::vector<std::vector<uint8_t>> txs(rng() % 4 == 0 ? 0 : rng() % 40);
        for (auto& t : txs) t = bytes(rng() % 8 == 0 ? 0 : rng() % 300);
        check_block(rr, txs, rng() % 2 == 0);
    }
    // the 4 GiB rule of the block encoder's 32-bit positions
    CHECK(hgx::block_text_fits(0) && hgx::block_text_fits(hgx::kBlockTextLimit - 1));
    CHECK(!hgx::block_text_fits(hgx::kBlockTextLimit) && !hgx::block_text_fits(-1));
    CHECK(hgx::block_text_bound(3, 0, 0) >= 3 * (17 + 20 + 16 + 6));
    CHECK(!hgx::block_text_fits(hgx::block_text_bound(1, 1, (int64_t)3 << 30)));   // 3 GiB is 4 GiB of base64
    CHECK(hgx::decimal_len(0) == 1 && hgx::decimal_len(-1) == 2 && hgx::decimal_len(INT64_MIN) == 20);
    CHECK(hgx::base64_len(0) == 0 && hgx::base64_len(1) == 4 && hgx::base64_len(3) == 4 && hgx::base64_len(4) == 8);
    // the growth plan
    for (int k = 0; k < 4000; k++) {
        const int64_t cap = (int64_t)(rng() >> (rng() % 40 + 20)), need = (int64_t)(rng() >> (rng() % 40 + 4));
        const int64_t got = hgx::body_grow_plan(cap, need);
        CHECK(got == grow_restated(cap, need));
        CHECK(got >= need && got >= cap && (got == cap || got < 2 * (need > hgx::kBodyMinCap ? need : hgx::kBodyMinCap)));
    }
    CHECK(hgx::body_grow_plan(0, 0) == 0 && hgx::body_grow_plan(0, 1) == hgx::kBodyMinCap);
    CHECK(hgx::body_grow_plan(2, 2) == 2 && hgx::body_grow_plan(2, 3) == hgx::kBodyMinCap);
    CHECK(hgx::body_grow_plan(4096, 4097) == 8192 && hgx::body_grow_plan(4096, 70000) == 131072);
    CHECK(hgx::body_grow_plan(5, -1) == -1 && hgx::body_grow_plan(-1, 5) == -1);
    CHECK(hgx::body_grow_plan(0, INT64_MAX) == -1);   // (no doubling passes 2^62)
    // the capacity rule: a NULL array has capacity 0; both must fit
    int64_t o[4];
    uint8_t b[4];
    CHECK(hgx::body_out_fits(3, 4, o, 3, b, 4) == 0);
    CHECK(hgx::body_out_fits(3, 4, o, 2, b, 4) == 1 && hgx::body_out_fits(3, 4, o, 3, b, 3) == 1);
    CHECK(hgx::body_out_fits(3, 4, nullptr, 3, b, 4) == 1 && hgx::body_out_fits(3, 4, o, 3, nullptr, 4) == 1);
    CHECK(hgx::body_out_fits(0, 0, nullptr, 0, nullptr, 0) == 0 && hgx::body_out_fits(1, 0, nullptr, 0, nullptr, 0) == 1);
    CHECK(hgx::body_out_fits(2, 0, o, 2, nullptr, 0) == 0);   // empty transactions need no byte array
    // hgx_keep_bodies
    CHECK(hgx::keep_bodies_check(true, 0, 0, 0, false, false) == nullptr);
    CHECK(hgx::keep_bodies_check(true, 0, 5, 7, false, false) == nullptr);
    CHECK(hgx::keep_bodies_check(false, 0, 0, 0, false, false) != nullptr);
    CHECK(hgx::keep_bodies_check(true, 1, 0, 0, false, false) != nullptr);
    CHECK(hgx::keep_bodies_check(true, 0, -1, 0, false, false) != nullptr);
    CHECK(hgx::keep_bodies_check(true, 0, 0, -1, false, false) != nullptr);
    CHECK(hgx::keep_bodies_check(true, 0, 0, 0, true, false) != nullptr);
    CHECK(hgx::keep_bodies_check(true, 0, 0, 0, false, true) != nullptr);
    std::printf("%d cases ok\n", cases);
    return 0;
}
