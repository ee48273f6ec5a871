// Stand-alone check of the version-3 checkpoint host side (babble_amd/csrc/hgx_ckpt_host.cpp, no HIP):
//  - seeded random valid images, rooted and unrooted, built by the writer below (its own code, section by
//    section as include/hgx.h lists them) must be accepted, and every parsed field must be the writer's;
//  - every truncation of an image must be refused: the bare prefix, and the prefix closed with a checksum
//    of its own;
//  - every single-field corruption, closed with a recomputed checksum, must be refused;
//  - the piece planner against a direct restatement over the writer's own arrays, for random limits, and
//    the pieces must tile [0, E);
//  - the pair search against a linear scan.
// Meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibabble_amd/csrc \
//       tools/ckpt_host_check.cpp babble_amd/csrc/hgx_ckpt_host.cpp -o ckpt_host_check && ./ckpt_host_check
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "hgx_ckpt_host.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);       \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

using Bytes = std::vector<uint8_t>;
using Id = std::array<uint8_t, 32>;

struct Image {
    Bytes b;                              // the file with its checksum
    std::map<std::string, size_t> at;     // where the named fields start
    int32_t n = 0, G = 0, flags = 0;
    int64_t E = 0, C = 0, T = 0;
    std::vector<int32_t> ntx;
    std::vector<uint8_t> nil;
    std::vector<int64_t> off;
    std::vector<Id> pair_event;
    int64_t n_blocks = 0;
};

static uint64_t fnv(const uint8_t* p, size_t n) {
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < n; i++) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}

static void close_image(Bytes& body) {   // body -> body | FNV-1a
    const uint64_t h = fnv(body.data(), body.size());
    const uint8_t* p = (const uint8_t*)&h;
    body.insert(body.end(), p, p + 8);
}

template <typename T>
static void put(Bytes& b, T v) {
    const uint8_t* p = (const uint8_t*)&v;
    b.insert(b.end(), p, p + sizeof(T));
}

static Id random_id(std::mt19937_64& rng) {
    Id x;
    for (auto& v : x) v = (uint8_t)rng();
    return x;
}

static Image make_image(uint64_t seed, bool rooted) {
    std::mt19937_64 rng(seed);
    Image im;
    im.n = 1 + (int32_t)(rng() % 5);
    im.G = rooted ? 1 : 1 + (int32_t)(rng() % 2);
    im.C = (int64_t)im.n * im.G;
    im.E = (int64_t)(rng() % 9);
    im.flags = 2 | 4 | 16 | (rooted ? 1 : 0);
    Bytes& b = im.b;
    const char magic[8] = {'H', 'G', 'X', 'C', 'K', 'P', 'T', '1'};
    b.insert(b.end(), magic, magic + 8);
    im.at["version"] = b.size(); put<uint32_t>(b, 3);
    im.at["n"] = b.size(); put<int32_t>(b, im.n);
    im.at["G"] = b.size(); put<int32_t>(b, im.G);
    im.at["flags"] = b.size(); put<int32_t>(b, im.flags);
    im.at["E"] = b.size(); put<int64_t>(b, im.E);
    const int64_t C = im.C, E = im.E;
    if (rooted) {
        std::vector<uint8_t> ry((size_t)C), hx((size_t)C);
        for (int64_t p = 0; p < C; p++) put<int32_t>(b, (int32_t)(rng() % 7) - 1);
        for (int64_t p = 0; p < C; p++) put<int32_t>(b, (int32_t)(rng() % 5) - 1);
        im.at["root_y"] = b.size();
        for (int64_t p = 0; p < C; p++) b.push_back(ry[(size_t)p] = (uint8_t)(rng() & 1));
        im.at["root_y_pad"] = b.size();
        while (b.size() % 4) b.push_back(0);   // (the header and the two columns before are multiples of 4)
        std::vector<Id> ev((size_t)(rng() % 4));
        for (auto& x : ev) x = random_id(rng);
        std::sort(ev.begin(), ev.end());
        im.pair_event = ev;
        im.at["n_others"] = b.size(); put<int64_t>(b, (int64_t)ev.size());
        im.at["others"] = b.size();
        for (auto& x : ev) b.insert(b.end(), x.begin(), x.end());
        im.n_blocks = (int64_t)(rng() % 4);
        put<int32_t>(b, 1); put<int32_t>(b, 4); put<int32_t>(b, 9); put<int32_t>(b, 0);
        put<int64_t>(b, 123);
        im.at["n_blocks"] = b.size(); put<int64_t>(b, im.n_blocks);
        for (int64_t k = 0; k < im.n_blocks; k++) {
            put<int32_t>(b, (int32_t)k); put<int32_t>(b, 3); put<int64_t>(b, 5); put<int32_t>(b, 0); put<int32_t>(b, 1);
        }
        im.at["has_x"] = b.size();
        for (int64_t p = 0; p < C; p++) b.push_back(hx[(size_t)p] = (uint8_t)(rng() & 1));
        im.at["has_y"] = b.size();
        for (int64_t p = 0; p < C; p++) b.push_back(ry[(size_t)p]);
        im.at["has_pad"] = b.size();
        for (int64_t k = 2 * C; k % 4; k++) b.push_back(0);
        im.at["x_id"] = b.size();
        for (int64_t p = 0; p < C; p++) {
            Id x = random_id(rng);
            x[0] |= 1;
            if (!hx[(size_t)p]) x.fill(0);
            b.insert(b.end(), x.begin(), x.end());
        }
        im.at["y_id"] = b.size();
        for (int64_t p = 0; p < C; p++) {
            Id x = random_id(rng);
            x[0] |= 1;
            if (!ry[(size_t)p]) x.fill(0);
            b.insert(b.end(), x.begin(), x.end());
        }
        im.at["n_pairs"] = b.size(); put<int64_t>(b, (int64_t)ev.size());
        im.at["pair_event"] = b.size();
        for (auto& x : ev) b.insert(b.end(), x.begin(), x.end());
        im.at["pair_parent"] = b.size();
        for (size_t k = 0; k < ev.size(); k++) {
            const Id x = random_id(rng);
            b.insert(b.end(), x.begin(), x.end());
        }
        im.at["block_hashes"] = b.size();
        for (int64_t k = 0; k < im.n_blocks; k++) {
            const bool has = k % 2 == 0;
            Id x = random_id(rng);
            x[0] |= 1;
            if (!has) x.fill(0);
            b.push_back(has ? 1 : 0); b.push_back(0); b.push_back(0); b.push_back(0);
            b.insert(b.end(), x.begin(), x.end());
        }
    }
    std::vector<Id> ids((size_t)E);
    for (auto& x : ids) x = random_id(rng);
    im.ntx.resize((size_t)E);
    im.nil.resize((size_t)E);
    for (int64_t i = 0; i < E; i++) {
        im.nil[(size_t)i] = rng() % 4 == 0;
        im.ntx[(size_t)i] = im.nil[(size_t)i] ? 0 : (int32_t)(rng() % 4);
        im.T += im.ntx[(size_t)i];
    }
    for (int64_t i = 0; i < E; i++) put<int32_t>(b, (int32_t)(rng() % (uint64_t)C));
    for (int col = 0; col < 4; col++)
        for (int64_t i = 0; i < E; i++) put<int64_t>(b, (int64_t)(rng() % 100) - 4);
    for (int64_t i = 0; i < 32 * E; i++) b.push_back((uint8_t)rng());
    im.at["coin"] = b.size();
    for (int64_t i = 0; i < E; i++) b.push_back(ids[(size_t)i][16] != 0);
    im.at["ntx"] = b.size();
    for (int64_t i = 0; i < E; i++) put<int32_t>(b, im.ntx[(size_t)i]);
    im.at["nil"] = b.size();
    for (int64_t i = 0; i < E; i++) b.push_back(im.nil[(size_t)i]);
    im.at["ids"] = b.size();
    for (auto& x : ids) b.insert(b.end(), x.begin(), x.end());
    for (int64_t i = 0; i < 65 * C; i++) b.push_back((uint8_t)rng());
    for (int64_t i = 0; i < 32 * E; i++) b.push_back((uint8_t)rng());
    im.at["T"] = b.size(); put<int64_t>(b, im.T);
    im.off.assign((size_t)im.T + 1, 0);
    for (int64_t t = 0; t < im.T; t++) im.off[(size_t)t + 1] = im.off[(size_t)t] + (int64_t)(rng() % 40);
    im.at["tx_off"] = b.size();
    for (int64_t v : im.off) put<int64_t>(b, v);
    im.at["tx_bytes"] = b.size();
    for (int64_t i = 0; i < im.off.back(); i++) b.push_back((uint8_t)rng());
    im.at["end"] = b.size();
    close_image(b);
    return im;
}

static bool accepted(const Bytes& file, int32_t n, int32_t G, hgx::Ckpt3* out = nullptr) {
    // an exact-size copy on the heap: a read past the image is a read past the allocation
    uint8_t* p = (uint8_t*)std::malloc(file.size() ? file.size() : 1);
    if (!file.empty()) std::memcpy(p, file.data(), file.size());
    hgx::Ckpt3 f;
    std::string why;
    const char* r = hgx::ckpt3_parse(p, file.size(), n, G, f, why);
    if (r) CHECK(!why.empty() && r == why.c_str());
    if (out && !r) {   // (the pointers of a caller that keeps the view must outlive it: re-parse the caller's bytes)
        CHECK(hgx::ckpt3_parse(file.data(), file.size(), n, G, *out, why) == nullptr);
    }
    std::free(p);
    return r == nullptr;
}

// the image with `bytes` at `pos` replaced (the body may grow by `extra` trailing bytes), closed again
static Bytes corrupt(const Image& im, size_t pos, const void* bytes, size_t nbytes, size_t extra = 0) {
    Bytes body(im.b.begin(), im.b.end() - 8);
    CHECK(pos + nbytes <= body.size());
    std::memcpy(body.data() + pos, bytes, nbytes);
    body.insert(body.end(), extra, 0);
    close_image(body);
    return body;
}

template <typename T>
static Bytes with(const Image& im, const char* field, int64_t index, T value) {
    return corrupt(im, im.at.at(field) + (size_t)index * sizeof(T), &value, sizeof(T));
}

static int check_corruptions(const Image& im) {
    int cases = 0;
    auto refuse = [&](const Bytes& f) {
        CHECK(!accepted(f, im.n, im.G));
        cases++;
    };
    refuse(with<uint32_t>(im, "version", 0, 2));
    refuse(with<uint32_t>(im, "version", 0, 4));
    for (int32_t bit : {2, 4, 16}) refuse(with<int32_t>(im, "flags", 0, im.flags & ~bit));
    for (int32_t bit : {8, 32, 1 << 30}) refuse(with<int32_t>(im, "flags", 0, im.flags | bit));
    refuse(with<int32_t>(im, "flags", 0, im.flags ^ 1));   // the rooted section appears or vanishes
    refuse(with<int32_t>(im, "n", 0, im.n + 1));
    refuse(with<int32_t>(im, "G", 0, im.G + 1));
    refuse(with<int32_t>(im, "n", 0, 0));
    refuse(with<int64_t>(im, "E", 0, im.E + 1));
    refuse(with<int64_t>(im, "E", 0, -1));
    refuse(with<int64_t>(im, "E", 0, INT64_MAX));
    if (im.E > 0) refuse(with<int64_t>(im, "E", 0, im.E - 1));
    refuse(with<int64_t>(im, "T", 0, im.T + 1));
    refuse(with<int64_t>(im, "T", 0, -1));
    refuse(with<int64_t>(im, "T", 0, INT64_MAX));
    refuse(with<int64_t>(im, "tx_off", 0, 1));
    if (im.T >= 2) refuse(with<int64_t>(im, "tx_off", 1, im.off.back() + 1));
    refuse(with<int64_t>(im, "tx_off", im.T, im.off.back() + 1));
    if (im.T >= 1) refuse(with<int64_t>(im, "tx_off", im.T, -1));
    {
        const uint8_t z = 0;
        refuse(corrupt(im, 0, &z, 0, 1));   // one byte too many
    }
    for (int64_t i = 0; i < im.E; i++) {
        refuse(with<int32_t>(im, "ntx", i, -1));
        refuse(with<int32_t>(im, "ntx", i, im.ntx[(size_t)i] + 1));
        refuse(with<uint8_t>(im, "nil", i, 2));
        if (im.ntx[(size_t)i] > 0) refuse(with<uint8_t>(im, "nil", i, 1));
        refuse(with<uint8_t>(im, "coin", i, im.b[im.at.at("coin") + (size_t)i] ^ 1));
    }
    if (!(im.flags & 1)) return cases;
    const int64_t C = im.C, np = (int64_t)im.pair_event.size();
    if (C % 4) refuse(with<uint8_t>(im, "root_y_pad", 0, 1));
    if ((2 * C) % 4) refuse(with<uint8_t>(im, "has_pad", 0, 1));
    refuse(with<int64_t>(im, "n_others", 0, np + 1));
    refuse(with<int64_t>(im, "n_others", 0, -1));
    refuse(with<int64_t>(im, "n_pairs", 0, np + 1));
    refuse(with<int64_t>(im, "n_pairs", 0, INT64_MAX));
    refuse(with<int64_t>(im, "n_blocks", 0, im.n_blocks + 1));
    refuse(with<int64_t>(im, "n_blocks", 0, -1));
    for (int64_t p = 0; p < C; p++) {
        const uint8_t hx = im.b[im.at.at("has_x") + (size_t)p], hy = im.b[im.at.at("has_y") + (size_t)p];
        refuse(with<uint8_t>(im, "has_x", p, 2));
        refuse(with<uint8_t>(im, "has_y", p, hy ^ 1));
        refuse(with<uint8_t>(im, "root_y", p, hy ^ 1));
        if (!hx) refuse(with<uint8_t>(im, "x_id", 32 * p + 31, 1));
        else refuse(with<uint8_t>(im, "has_x", p, 0));   // (its id row is not zero)
        if (!hy) refuse(with<uint8_t>(im, "y_id", 32 * p, 1));
    }
    for (int64_t j = 0; j < np; j++) {
        refuse(with<uint8_t>(im, "pair_event", 32 * j + 7, im.pair_event[(size_t)j][7] ^ 0x10));
        refuse(with<uint8_t>(im, "others", 32 * j + 7, im.pair_event[(size_t)j][7] ^ 0x10));
    }
    if (np >= 2) {   // both sections in the same wrong order
        Bytes body(im.b.begin(), im.b.end() - 8);
        for (const char* sec : {"others", "pair_event"}) {
            uint8_t* p = body.data() + im.at.at(sec);
            std::swap_ranges(p, p + 32, p + 32);
        }
        close_image(body);
        refuse(body);
    }
    for (int64_t k = 0; k < im.n_blocks; k++) {
        const bool has = im.b[im.at.at("block_hashes") + 36 * (size_t)k] != 0;
        refuse(with<uint8_t>(im, "block_hashes", 36 * k, 2));
        refuse(with<uint8_t>(im, "block_hashes", 36 * k + 2, 1));
        if (!has) refuse(with<uint8_t>(im, "block_hashes", 36 * k + 9, 1));
        else refuse(with<uint8_t>(im, "block_hashes", 36 * k, 0));
    }
    return cases;
}

static void check_fields(const Image& im) {
    hgx::Ckpt3 f;
    CHECK(accepted(im.b, im.n, im.G, &f));
    CHECK(accepted(im.b, 0, 0));
    CHECK(f.n == im.n && f.G == im.G && f.E == im.E && f.C == im.C && f.flags == im.flags && f.T == im.T);
    CHECK(f.n_bytes == im.off.back());
    for (int64_t i = 0; i < im.E; i++) {
        CHECK(hgx::ckpt_rd<int32_t>(f.ntx, i) == im.ntx[(size_t)i]);
        CHECK(f.nil[i] == im.nil[(size_t)i]);
    }
    for (int64_t t = 0; t <= im.T; t++) CHECK(hgx::ckpt_rd<int64_t>(f.tx_off, t) == im.off[(size_t)t]);
    CHECK(f.tx_bytes == im.b.data() + im.at.at("tx_bytes"));
    CHECK(f.ids == im.b.data() + im.at.at("ids"));
    if (im.flags & 1) {
        CHECK(f.n_pairs == (int64_t)im.pair_event.size() && f.n_others == f.n_pairs);
        CHECK((int64_t)f.kept.size() == im.G && f.kept[0].n_blocks == im.n_blocks && f.kept[0].consensus_tx == 123);
        CHECK(f.kept[0].has_lcr == 1 && f.kept[0].lcr == 4 && f.kept[0].lcre == 9);
        CHECK(f.pair_event == im.b.data() + im.at.at("pair_event"));
        CHECK(f.kept[0].hashes == im.b.data() + im.at.at("block_hashes"));
        // the pair search against a linear scan: every key, and ids that are no key
        std::mt19937_64 rng(im.E + 77);
        for (size_t j = 0; j < im.pair_event.size(); j++) CHECK(hgx::ckpt3_find_pair(f, im.pair_event[j].data()) == (int64_t)j);
        for (int k = 0; k < 20; k++) {
            const Id x = random_id(rng);
            int64_t want = -1;
            for (size_t j = 0; j < im.pair_event.size(); j++)
                if (im.pair_event[j] == x) want = (int64_t)j;
            CHECK(hgx::ckpt3_find_pair(f, x.data()) == want);
        }
    } else {
        CHECK(f.kept.empty() && !f.has_x && !f.pair_event && f.n_pairs == 0);
    }
}

static int check_planner(const Image& im, std::mt19937_64& rng) {
    hgx::Ckpt3 f;
    CHECK(accepted(im.b, im.n, im.G, &f));
    int cases = 0;
    for (int round = 0; round < 40; round++) {
        const int64_t max_events = 1 + (int64_t)(rng() % 5), max_bytes = (int64_t)(rng() % 90);
        int64_t lo = 0, t_lo = 0;
        while (lo < im.E) {
            // the restatement: grow the piece one event at a time over the writer's own arrays
            int64_t want = lo, t = t_lo;
            while (want < im.E && want - lo < max_events) {
                const int64_t t1 = t + im.ntx[(size_t)want];
                if (want > lo && im.off[(size_t)t1] - im.off[(size_t)t_lo] > max_bytes) break;
                t = t1;
                want++;
            }
            int64_t hi = -1, t_hi = -1;
            hgx::ckpt3_piece(f, lo, t_lo, max_events, max_bytes, &hi, &t_hi);
            CHECK(hi == want && t_hi == t && hi > lo);
            lo = hi;
            t_lo = t_hi;
            cases++;
        }
        CHECK(lo == im.E && t_lo == im.T);
    }
    int64_t hi = 5, t_hi = 5;   // outside the file: nothing is read, nothing advances
    hgx::ckpt3_piece(f, im.E, im.T, 4, 100, &hi, &t_hi);
    CHECK(hi == im.E && t_hi == im.T);
    hgx::ckpt3_piece(f, -1, 0, 4, 100, &hi, &t_hi);
    CHECK(hi == -1);
    return cases;
}

int main() {
    int images = 0, cuts = 0, corruptions = 0, pieces = 0;
    std::mt19937_64 rng(2024);
    for (uint64_t seed = 1; seed <= 24; seed++) {
        const Image im = make_image(seed, seed % 2 == 0);
        check_fields(im);
        images++;
        corruptions += check_corruptions(im);
        pieces += check_planner(im, rng);
        if (seed > 8) continue;   // (quadratic in the image's size)
        for (size_t len = 0; len < im.b.size(); len++) {
            Bytes cut(im.b.begin(), im.b.begin() + (long)len);
            CHECK(!accepted(cut, im.n, im.G));
            if (len + 8 < im.b.size()) {   // a shorter body with a checksum of its own
                close_image(cut);
                CHECK(!accepted(cut, im.n, im.G));
            }
            cuts++;
        }
    }
    {
        hgx::Ckpt3 f;
        std::string why;
        CHECK(hgx::ckpt3_parse(nullptr, 0, 0, 0, f, why) != nullptr);
    }
    std::printf("%d images ok, %d truncations, %d corruptions and %d pieces checked\n", images, cuts, corruptions, pieces);
    return 0;
}
