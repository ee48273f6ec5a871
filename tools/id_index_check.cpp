// Stand-alone check of the event-id index's contract (babble_amd/csrc/hgx_idindex.h), host side only:
// no HIP, no context. Meant for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ibabble_amd/csrc
//       tools/id_index_check.cpp -o id_index_check
// Seeded random key sets go through the header's sequential model: every inserted key is found under
// its lowest value, absent keys are not, and the statistics hgx_id_index_state reports (entries, summed
// displacement, entries below their home slot) are the same under shuffled insertion orders, which is
// what lets the GPU tests pin them although the device inserts concurrently. Also: a cluster that
// wraps past the last slot, duplicate keys, a full table (the bounded probe), the sizing rule.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "hgx_idindex.h"

using namespace hgx;

static int g_fail = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
            g_fail++;                                                   \
        }                                                               \
    } while (0)

struct Table {
    uint64_t slots;
    std::vector<uint64_t> tab;
    std::vector<uint8_t> rows;   // [n][32]
    int64_t n = 0;
    explicit Table(uint64_t s) : slots(s), tab(s, 0) {}
    void add_row(const uint8_t* id) {
        rows.insert(rows.end(), id, id + 32);
        n++;
    }
    // rows first, then the values in `order` (the device inserts rows that are already in the column)
    bool insert_all(const std::vector<int64_t>& order) {
        for (int64_t v : order)
            if (!idx_model_insert(tab.data(), slots, rows.data() + 32 * v, v)) return false;
        return true;
    }
    int64_t find(const uint8_t* id, int64_t limit) const { return idx_probe(tab.data(), slots, rows.data(), n, id, limit); }
    IdxStats stats(bool* ok) const {
        IdxStats st;
        *ok = true;
        for (uint64_t s = 0; s < slots; s++) {
            if (!tab[s]) continue;
            uint64_t d = 0, w = 0;
            if (!idx_slot_stats(tab.data(), slots, rows.data(), n, s, &d, &w)) *ok = false;
            st.entries++;
            st.displacement += d;
            st.wrapped += w;
        }
        return st;
    }
};

static void random_id(std::mt19937_64& rng, uint8_t* id) {
    for (int w = 0; w < 4; w++) {
        const uint64_t x = rng();
        std::memcpy(id + 8 * w, &x, 8);
    }
}

static void set_home(uint8_t* id, uint64_t home) {   // bytes 0..7, little-endian
    for (int b = 0; b < 8; b++) id[b] = (uint8_t)(home >> (8 * b));
}

static void check_sizing() {
    const int64_t caps[] = {1, 2, 3, 63, 64, 65};
    const uint64_t want[] = {2, 4, 8, 128, 128, 256};
    for (int i = 0; i < 6; i++) {
        const uint64_t s = idx_slots_for(caps[i]);
        CHECK(s == want[i]);
        CHECK((s & (s - 1)) == 0 && s >= 2 * (uint64_t)caps[i] && (s / 2 < 2 * (uint64_t)caps[i] || s == 2));
    }
    CHECK(idx_slots_for(10000000) == (1ull << 25));   // 256 MiB of 8-byte words
}

static void check_contract_bytes() {
    uint8_t id[32];
    for (int b = 0; b < 32; b++) id[b] = (uint8_t)(b + 1);
    CHECK(idx_home(id, 1ull << 16) == 0x0201u);
    CHECK(idx_home(id, 128) == 0x01u);
    CHECK(idx_tag(id) == 0x0C0B0A09u);
    const uint64_t w = idx_word(idx_tag(id), 41);
    CHECK(w == ((0x0C0B0A09ull << 32) | 42) && idx_word_tag(w) == 0x0C0B0A09u && idx_word_value(w) == 41);
    CHECK(idx_word(0, 0) != 0);   // a stored word is never the empty word
    CHECK(idx_displacement(1, 126, 128) == 3 && idx_displacement(5, 5, 128) == 0);
}

static int random_sets(int cases) {
    std::mt19937_64 rng(20240917);
    int wrapped_cases = 0;
    for (int c = 0; c < cases; c++) {
        const int64_t cap = 1 + (int64_t)(rng() % 200);
        const uint64_t slots = idx_slots_for(cap);
        const int64_t n = 1 + (int64_t)(rng() % (uint64_t)cap);
        Table t(slots);
        uint8_t id[32];
        for (int64_t k = 0; k < n; k++) {
            random_id(rng, id);
            if (c % 3 == 0) set_home(id, slots - 1 - (rng() % 3));   // crowd the last slots: clusters that wrap
            if (c % 5 == 0 && k > 0 && rng() % 4 == 0) std::memcpy(id, t.rows.data() + 32 * (rng() % (uint64_t)k), 32);   // a repeated key
            t.add_row(id);
        }
        std::vector<int64_t> order((size_t)n);
        std::iota(order.begin(), order.end(), 0);
        CHECK(t.insert_all(order));
        bool ok = false;
        const IdxStats st0 = t.stats(&ok);
        CHECK(ok && st0.entries == (uint64_t)n);
        wrapped_cases += st0.wrapped > 0;
        // every key under its lowest value; with a limit, the lowest below it
        for (int64_t k = 0; k < n; k++) {
            int64_t low = k;
            for (int64_t j = 0; j < k; j++)
                if (!std::memcmp(t.rows.data() + 32 * j, t.rows.data() + 32 * k, 32)) { low = j; break; }
            CHECK(t.find(t.rows.data() + 32 * k, n) == low);
            CHECK(t.find(t.rows.data() + 32 * k, low) == kIdxNone);      // (nothing earlier holds it)
            CHECK(t.find(t.rows.data() + 32 * k, low + 1) == low);
        }
        // absent keys: random, a last byte flipped, the same home and tag with another row
        for (int q = 0; q < 16; q++) {
            random_id(rng, id);
            CHECK(t.find(id, n) == kIdxNone);
            std::memcpy(id, t.rows.data() + 32 * (rng() % (uint64_t)n), 32);
            id[31] ^= 1;
            bool present = false;
            for (int64_t j = 0; j < n; j++) present |= !std::memcmp(t.rows.data() + 32 * j, id, 32);
            if (!present) CHECK(t.find(id, n) == kIdxNone);
            id[31] ^= 1;
            id[12 + q % 19] ^= 0x80;   // bytes 0..11 (home and tag) stay
            present = false;
            for (int64_t j = 0; j < n; j++) present |= !std::memcmp(t.rows.data() + 32 * j, id, 32);
            if (!present) CHECK(t.find(id, n) == kIdxNone);
        }
        // the statistics and the occupied slots under shuffled insertion orders
        for (int rep = 0; rep < 4; rep++) {
            std::shuffle(order.begin(), order.end(), rng);
            Table u(slots);
            u.rows = t.rows;
            u.n = n;
            CHECK(u.insert_all(order));
            const IdxStats st = u.stats(&ok);
            CHECK(ok && st.entries == st0.entries && st.displacement == st0.displacement && st.wrapped == st0.wrapped);
            for (uint64_t s = 0; s < slots; s++) CHECK((u.tab[s] != 0) == (t.tab[s] != 0));
            for (int64_t k = 0; k < n; k += 7) CHECK(u.find(t.rows.data() + 32 * k, n) == t.find(t.rows.data() + 32 * k, n));
        }
    }
    return wrapped_cases;
}

static void check_wrap_cluster() {
    // 8 slots, five keys at home 6: slots 6, 7, 0, 1, 2; a key at home 0 then lands at 3
    Table t(8);
    uint8_t id[32] = {};
    for (int k = 0; k < 5; k++) {
        id[20] = (uint8_t)k;
        set_home(id, 6);
        t.add_row(id);
    }
    id[20] = 9;
    set_home(id, 0);
    t.add_row(id);
    CHECK(t.insert_all({0, 1, 2, 3, 4, 5}));
    const uint64_t occ[] = {1, 1, 1, 1, 0, 0, 1, 1};
    for (int s = 0; s < 8; s++) CHECK((t.tab[s] != 0) == (occ[s] != 0));
    bool ok = false;
    const IdxStats st = t.stats(&ok);
    CHECK(ok && st.entries == 6 && st.wrapped == 3 && st.displacement == 0 + 1 + 2 + 3 + 4 + 3);
    for (int k = 0; k < 6; k++) CHECK(t.find(t.rows.data() + 32 * k, 6) == k);
    id[20] = 77;   // absent, home at the last slot: the probe walks 7, 0, 1, 2, 3 and ends at 4
    set_home(id, 7);
    CHECK(t.find(id, 6) == kIdxNone);
}

static void check_full_table() {
    // more keys than slots cannot happen behind the sizing rule; the probes still end
    Table t(4);
    uint8_t id[32] = {};
    for (int k = 0; k < 5; k++) {
        id[16] = (uint8_t)(k + 1);
        set_home(id, (uint64_t)k);
        t.add_row(id);
    }
    CHECK(t.insert_all({0, 1, 2, 3}));
    CHECK(!idx_model_insert(t.tab.data(), 4, t.rows.data() + 32 * 4, 4));
    CHECK(t.find(t.rows.data() + 32 * 4, 5) == kIdxCorrupt);   // no empty slot ends the scan
    // a word naming no row
    Table u(4);
    u.add_row(t.rows.data());
    u.tab[idx_home(u.rows.data(), 4)] = idx_word(idx_tag(u.rows.data()), 3);
    CHECK(u.find(u.rows.data(), 1) == kIdxCorrupt);
    bool ok = true;
    (void)u.stats(&ok);
    CHECK(!ok);
}

int main() {
    check_sizing();
    check_contract_bytes();
    check_wrap_cluster();
    check_full_table();
    const int cases = 300;
    const int wrapped = random_sets(cases);
    CHECK(wrapped > 20);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("id index: %d random key sets ok (%d with a wrapped cluster), sizing, wrap, full table ok\n", cases, wrapped);
    return 0;
}
