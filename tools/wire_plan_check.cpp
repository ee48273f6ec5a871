// Stand-alone check of hgx_insert_wire_bodies' host plan (babble_amd/csrc/hgx_wire_plan_host.cpp, no
// HIP): 480 seeded random (resident chains, wire batch) cases against a direct restatement of
// ReadWireInfo (hashgraph.go:569-614) over RollingIndex.GetItem (common/rolling_index.go:40-50), which
// here materialises every participant's item list (the gids) and appends the batch's events to it one
// by one. The window kernel is restated on the host too (every resident event at or above its creator's
// lo writes its gid to its slot), so a descriptor is followed to the gid it stands for. Meant for the
// host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibabble_amd/csrc \
//       tools/wire_plan_check.cpp babble_amd/csrc/hgx_wire_plan_host.cpp -o wire_plan_check && ./wire_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "hgx.h"
#include "hgx_wire_plan.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s (line %d, case %d)\n", #x, __LINE__, g_case); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static int g_case = 0;

// Go's string(int) for the values the cases use (below 0x800) and the replacement rune for negatives
static std::string rune(int64_t v) {
    std::string s;
    if (v < 0) return "\xEF\xBF\xBD";
    if (v < 0x80) s += (char)v;
    else { s += (char)(0xC0 | (v >> 6)); s += (char)(0x80 | (v & 63)); }
    return s;
}

// RollingIndex with its items spelled out (the gid of every cached event)
struct Rolling {
    int64_t lastIndex = -1;
    std::vector<int64_t> items;
    // GetItem(index): 0 ok, else the StoreErr type + 1
    int get_item(int64_t index, int64_t* gid) const {
        const int64_t n = (int64_t)items.size();
        const int64_t oldestCached = lastIndex - n + 1;
        if (index < oldestCached) return HGX_ERR_TOO_LATE;
        const int64_t findex = index - oldestCached;
        if (findex >= n) return HGX_ERR_KEY_NOT_FOUND;
        *gid = items[(size_t)findex];
        return 0;
    }
    void add(int64_t gid, int64_t index) {   // (the batch's earlier events count as inserted)
        items.push_back(gid);
        lastIndex = index;
    }
};

int main() {
    std::mt19937_64 rng(314);
    int64_t n_ok = 0, n_late = 0, n_late_pruned = 0, n_nf = 0, n_fwd = 0, n_panic_cr = 0, n_panic_op = 0, n_empty = 0,
            n_inbatch = 0, n_resident = 0, n_nowin = 0, n_levels_deep = 0;
    const int kCases = 480;
    for (int it = 0; it < kCases; it++) {
        g_case = it;
        const int n = 1 + (int)(rng() % (it % 9 == 0 ? 1024 : 10));
        // the resident chains, their events interleaved in a random gid order
        std::vector<Rolling> chains((size_t)n);
        std::vector<int32_t> last((size_t)n), len((size_t)n), first((size_t)n);
        std::vector<int32_t> todo;
        bool any_empty = false, any_pruned = false;
        for (int c = 0; c < n; c++) {
            const int items = rng() % 4 == 0 ? 0 : 1 + (int)(rng() % 30);
            first[(size_t)c] = rng() % 3 == 0 ? (int)(rng() % 40) : 0;   // a shortened (pruned) chain starts above 0
            len[(size_t)c] = items;
            last[(size_t)c] = items ? first[(size_t)c] + items - 1 : (rng() % 2 ? -1 : first[(size_t)c] - 1);
            chains[(size_t)c].lastIndex = last[(size_t)c];
            for (int k = 0; k < items; k++) todo.push_back(c);
            any_empty |= items == 0;
            any_pruned |= items > 0 && first[(size_t)c] > 0;
        }
        std::shuffle(todo.begin(), todo.end(), rng);
        const int64_t E0 = (int64_t)todo.size();
        std::vector<int32_t> g_creator((size_t)E0), g_index((size_t)E0);
        for (int64_t g = 0; g < E0; g++) {
            const int c = todo[(size_t)g];
            g_creator[(size_t)g] = c;
            g_index[(size_t)g] = first[(size_t)c] + (int32_t)chains[(size_t)c].items.size();
            chains[(size_t)c].items.push_back(g);
        }
        // the batch: mostly well-formed gossip, one fault of a random kind in about half of the cases
        const int64_t count = it % 16 == 0 ? 0 : 1 + (int64_t)(rng() % 60);
        const int fault = (int)(rng() % 12);   // 0 too late, 1 above the head, 2 forward reference, 3 / 4 panics
        const int64_t fault_at = count ? (int64_t)(rng() % (uint64_t)count) : -1;
        std::vector<int32_t> cr((size_t)count), opc((size_t)count);
        std::vector<int64_t> idx((size_t)count), spi((size_t)count), opi((size_t)count);
        {
            std::vector<int64_t> head((size_t)n);   // the Index each creator's next event gets
            std::vector<int64_t> oldest((size_t)n), items((size_t)n);
            for (int c = 0; c < n; c++) {
                head[(size_t)c] = last[(size_t)c] + 1;
                items[(size_t)c] = len[(size_t)c];
            }
            for (int64_t k = 0; k < count; k++) {
                const int c = (int)(rng() % (uint64_t)n);
                cr[(size_t)k] = c;
                idx[(size_t)k] = head[(size_t)c];
                spi[(size_t)k] = items[(size_t)c] ? head[(size_t)c] - 1 : -1;
                const int oc = (int)(rng() % (uint64_t)n);
                opc[(size_t)k] = oc;
                if (rng() % 5 == 0 || items[(size_t)oc] == 0) {
                    opi[(size_t)k] = -1 - (int64_t)(rng() % 3);
                    if (rng() % 2) opc[(size_t)k] = (int32_t)(rng() % 5000) - 2500;   // not read
                } else {   // any cached event of oc, the newest ones more often
                    const int64_t span = rng() % 3 ? std::min<int64_t>(items[(size_t)oc], 4) : items[(size_t)oc];
                    opi[(size_t)k] = head[(size_t)oc] - 1 - (int64_t)(rng() % (uint64_t)span);
                }
                if (k == fault_at) {
                    const int64_t old_oc = head[(size_t)oc] - items[(size_t)oc];
                    if (fault == 0 && old_oc >= 1) opi[(size_t)k] = old_oc - 1 - (int64_t)(rng() % (uint64_t)old_oc);
                    else if (fault == 1) opi[(size_t)k] = head[(size_t)oc] + (int64_t)(rng() % 3);
                    else if (fault == 2) opi[(size_t)k] = head[(size_t)oc];   // an event a later position may bring
                    else if (fault == 3) cr[(size_t)k] = rng() % 2 ? -1 - (int32_t)(rng() % 4) : n + (int32_t)(rng() % 4);
                    else if (fault == 4) { opc[(size_t)k] = rng() % 2 ? -1 : n; opi[(size_t)k] = (int64_t)(rng() % 5); }
                    else if (fault == 5 && items[(size_t)c]) spi[(size_t)k] = head[(size_t)c] - items[(size_t)c] - 1;
                }
                if (cr[(size_t)k] >= 0 && cr[(size_t)k] < n) {
                    head[(size_t)cr[(size_t)k]] = idx[(size_t)k] + 1;
                    items[(size_t)cr[(size_t)k]]++;
                }
            }
        }
        // ReadWireInfo per event, the reference way
        std::vector<Rolling> st = chains;
        std::vector<int64_t> want_sp, want_op;
        int64_t want_m = count;
        int32_t want_code = 0;
        std::string want_msg;
        bool forward = false;
        for (int64_t k = 0; k < count && !want_code; k++) {
            const int32_t c = cr[(size_t)k];
            int64_t s = -1, o = -1;
            if (c < 0 || c >= n) {
                want_code = HGX_ERR_PANIC;
                want_msg = "runtime error: slice bounds out of range [2:0]";
            }
            auto lookup = [&](int32_t p, int64_t index, int64_t* gid) {
                if (p < 0 || p >= n) {
                    want_code = HGX_ERR_PANIC;
                    want_msg = "runtime error: invalid memory address or nil pointer dereference";
                    return;
                }
                const int rc = st[(size_t)p].get_item(index, gid);
                if (rc) {
                    want_code = rc;
                    want_msg = rune(index) + (rc == HGX_ERR_TOO_LATE ? ", Too Late" : ", Not Found");
                }
            };
            if (!want_code && spi[(size_t)k] >= 0) lookup(c, spi[(size_t)k], &s);
            if (!want_code && opi[(size_t)k] >= 0) lookup(opc[(size_t)k], opi[(size_t)k], &o);
            if (want_code) {
                want_m = k;
                if (want_code == HGX_ERR_KEY_NOT_FOUND)   // does a later position bring that (creator, Index)?
                    for (int64_t j = k + 1; j < count; j++)
                        forward |= cr[(size_t)j] == opc[(size_t)k] && idx[(size_t)j] == opi[(size_t)k];
                break;
            }
            want_sp.push_back(s);
            want_op.push_back(o);
            st[(size_t)c].add(E0 + k, idx[(size_t)k]);
        }
        // the plan
        hgx::WirePlan p;
        hgx::wire_plan(hgx::WireIn{cr.data(), idx.data(), spi.data(), opc.data(), opi.data()}, count, last.data(),
                       len.data(), n, E0, p);
        CHECK(p.m == want_m && p.code == want_code && p.msg == want_msg);
        CHECK((int64_t)p.sp.size() == want_m && (int64_t)p.op.size() == want_m && (int64_t)p.level.size() == want_m);
        CHECK((int)p.lo.size() == n && (int)p.woff.size() == n);
        // the windows: disjoint, inside [0, slots), each [lo, last]; nobody named -> none
        int64_t run = 0;
        for (int c = 0; c < n; c++) {
            CHECK(p.woff[(size_t)c] == run);
            if (p.lo[(size_t)c] == hgx::kWireNoWindow) { n_nowin++; continue; }
            CHECK(len[(size_t)c] > 0 && p.lo[(size_t)c] >= first[(size_t)c] && p.lo[(size_t)c] <= last[(size_t)c]);
            run += last[(size_t)c] - p.lo[(size_t)c] + 1;
        }
        CHECK(p.slots == run && p.slots <= E0);
        // k_wire_window, restated: one writer per slot
        std::vector<int64_t> win((size_t)p.slots, -1);
        for (int64_t g = 0; g < E0; g++) {
            const int c = g_creator[(size_t)g];
            if (g_index[(size_t)g] < p.lo[(size_t)c]) continue;
            const int64_t slot = (int64_t)p.woff[(size_t)c] + g_index[(size_t)g] - p.lo[(size_t)c];
            CHECK(slot >= 0 && slot < p.slots && win[(size_t)slot] == -1);
            win[(size_t)slot] = g;
        }
        for (int64_t s = 0; s < p.slots; s++) CHECK(win[(size_t)s] >= 0);
        // every descriptor stands for the reference's gid; levels by hgx_batch_levels' rule on those gids
        int64_t resident = 0;
        int32_t top = 0;
        std::vector<int32_t> level((size_t)want_m);
        bool named_lo_hit = false;
        for (int64_t k = 0; k < want_m; k++) {
            auto gid_of = [&](int64_t d) {
                if (d >= -1) {
                    n_inbatch += d >= 0;
                    CHECK(d == -1 || (d >= E0 && d < E0 + k));
                    return d;
                }
                const int64_t slot = -2 - d;
                CHECK(slot < p.slots);
                resident++;
                return win[(size_t)slot];
            };
            const int64_t s = gid_of(p.sp[(size_t)k]), o = gid_of(p.op[(size_t)k]);
            CHECK(s == want_sp[(size_t)k] && o == want_op[(size_t)k]);
            int32_t l = 0;
            if (s >= E0) l = level[(size_t)(s - E0)] + 1;
            if (o >= E0) l = std::max(l, level[(size_t)(o - E0)] + 1);
            level[(size_t)k] = l;
            top = std::max(top, l + 1);
            CHECK(p.level[(size_t)k] == l);
            for (int64_t g : {s, o})
                if (g >= 0 && g < E0) named_lo_hit |= g_index[(size_t)g] == p.lo[(size_t)g_creator[(size_t)g]];
        }
        CHECK(p.n_levels == top && p.n_resident == resident);
        CHECK(resident == 0 ? p.slots == 0 : named_lo_hit);   // lo is an Index somebody names
        n_resident += resident;
        n_levels_deep += top >= 4;
        n_empty += any_empty && want_m > 0;
        if (!want_code) n_ok++;
        else if (want_code == HGX_ERR_TOO_LATE) { n_late++; n_late_pruned += any_pruned; }
        else if (want_code == HGX_ERR_KEY_NOT_FOUND) { n_nf++; n_fwd += forward; }
        else if (want_msg[15] == 's') n_panic_cr++;
        else n_panic_op++;
    }
    // nothing at all
    hgx::WirePlan p;
    hgx::wire_plan(hgx::WireIn{nullptr, nullptr, nullptr, nullptr, nullptr}, 0, nullptr, nullptr, 0, 0, p);
    CHECK(p.m == 0 && p.code == 0 && p.slots == 0 && p.sp.empty() && p.lo.empty());
    CHECK(hgx::wire_go_rune(3) == "\x03" && hgx::wire_go_rune(0x7FF) == "\xDF\xBF" && hgx::wire_go_rune(-1) == "\xEF\xBF\xBD");
    CHECK(n_ok > 150 && n_late > 8 && n_late_pruned > 3 && n_nf > 20 && n_fwd > 3 && n_panic_cr > 8 && n_panic_op > 8);
    CHECK(n_empty > 50 && n_inbatch > 1000 && n_resident > 1000 && n_nowin > 100 && n_levels_deep > 50);
    std::printf("wire_plan_check: %d cases ok (%lld clean, %lld too late (%lld on shortened chains), %lld not found "
                "(%lld forward references), %lld + %lld panics, %lld with empty chains, %lld in-batch and %lld resident "
                "parents, %lld creators without a window)\n",
                kCases, (long long)n_ok, (long long)n_late, (long long)n_late_pruned, (long long)n_nf, (long long)n_fwd,
                (long long)n_panic_cr, (long long)n_panic_op, (long long)n_empty, (long long)n_inbatch,
                (long long)n_resident, (long long)n_nowin);
    return 0;
}
