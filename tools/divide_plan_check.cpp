// Stand-alone check of DivideRounds' host plan (babble_amd/csrc/hgx_divide_plan_host.cpp, no HIP):
// 480 seeded sequences of calls on contexts of 1 to 1 024 chains (several graphs, odd n, silent
// chains, chains based near the uint16 coordinates' limit). Chains grow by random amounts, the
// previous call's lengths and slots carry over, and the round boundaries are a random table that
// is non-decreasing in r for every chain. Every call's plan is compared with a direct statement of
// each rule (r_lo: a linear scan), every rebuilt layout with the three properties the kernels rely
// on, and the round path's choice with its properties over every combination of its inputs.
// Meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ibabble_amd/csrc
//       tools/divide_plan_check.cpp babble_amd/csrc/hgx_divide_plan_host.cpp -o divide_plan_check
//   ./divide_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hgx_divide_plan.h"

using namespace hgx;

static int g_seq = 0, g_call = 0;

#define CHECK(x)                                                                              \
    do {                                                                                      \
        if (!(x)) {                                                                           \
            std::printf("FAILED %s (line %d, sequence %d, call %d)\n", #x, __LINE__, g_seq, g_call); \
            std::exit(1);                                                                     \
        }                                                                                     \
    } while (0)

static bool persistent(RoundPath p) { return p == RoundPath::Persistent || p == RoundPath::PersistentBig; }

// the round path over every combination of its inputs: properties, not a copy of the table
static int check_round_path() {
    int combos = 0;
    const int C = 48;
    const int64_t news[4] = {0, 6 * C - 1, 6 * C, 1000000};
    for (int k = 0; k <= 5; k++)
        for (int bits = 0; bits < 128; bits++)
            for (int64_t ne : news) {
                RoundPathIn in{};
                in.round_kernel = k;
                in.rooted = bits & 1; in.sharded = bits & 2; in.rebuild = bits & 4; in.round_pb_enabled = bits & 8;
                in.g_ok = bits & 16; in.p_ok = bits & 32; in.pb_ok = bits & 64;
                in.new_events = ne; in.C = C;
                const RoundChoice rc = round_path(in);
                combos++;
                const bool pb_usable = in.pb_ok && in.round_pb_enabled && !in.sharded;
                // a rooted context always steps with the per-candidate kernel
                if (in.rooted) CHECK(rc.path == RoundPath::Steps && rc.step_kernel == 0);
                // a sharded context never takes the whole-graph path, and the persistent one whenever round_p_ok
                if (in.sharded) CHECK(rc.path != RoundPath::WholeGraph);
                if (in.sharded && !in.rooted && in.p_ok) CHECK(rc.path == RoundPath::Persistent);
                if (in.sharded) CHECK(rc.path != RoundPath::PersistentBig);
                // modes 1 and 2 never launch a persistent kernel or the whole-graph one (outside a sharded group)
                if ((k == 1 || k == 2) && !in.sharded) CHECK(rc.path == RoundPath::Steps);
                // mode 0 takes a persistent path only on a rebuild, mode 3 on every call
                if (k == 0 && !in.sharded && !in.rebuild) CHECK(!persistent(rc.path));
                if (k == 0 && in.rebuild && !in.rooted && !in.g_ok && (in.p_ok || pb_usable)) CHECK(persistent(rc.path));
                if (k == 3 && !in.rooted && (in.p_ok || pb_usable)) CHECK(persistent(rc.path));
                if (persistent(rc.path)) CHECK(in.p_ok || pb_usable);
                if (rc.path == RoundPath::PersistentBig) CHECK(!in.p_ok && pb_usable);
                if (rc.path == RoundPath::WholeGraph) CHECK(in.g_ok && (k == 0 || k == 4));
                // the resumed calls' graphs are captured ahead only by a mode-0 rebuild that ran persistently
                CHECK(rc.precapture == (persistent(rc.path) && in.rebuild && k == 0));
                // nb is kStepBatch exactly on rebuilds; a resumed call replays 2 steps below 6 new events per chain, else 4
                CHECK((rc.nb == kStepBatch) == in.rebuild);
                if (!in.rebuild) CHECK(rc.nb == (ne < 6 * C ? kStepBatchSmall : 2 * kStepBatchSmall));
                CHECK(rc.step_graph == (in.rebuild ? 0 : rc.nb == kStepBatchSmall ? 1 : 2));
                CHECK(rc.step_kernel == ((k == 1 && !in.rooted) ? 1 : 0));
            }
    return combos;
}

int main() {
    std::mt19937_64 rng(1463);
    auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    const int ns[] = {1, 2, 3, 4, 5, 7, 16, 17, 33, 64, 128, 255, 256, 341, 512, 896, 897, 1000, 1023, 1024};
    const int seg = 16;
    long calls = 0, first = 0, flip_up = 0, flip_down = 0, outgrown = 0, inc_off = 0, resumed_hi = 0, resumed_no_old = 0,
         no_growth = 0, lanes_fit = 0, lanes_over = 0, layouts = 0;
    DividePlan plan;   // reused, as the engine's
    for (g_seq = 0; g_seq < 480; g_seq++) {
        const int n = ns[g_seq % (sizeof(ns) / sizeof(ns[0]))];
        const int G = n > 896 ? 1 : (int)rnd(1, std::min(4, 1024 / n));
        const int C = n * G;
        const int64_t cap = rnd(2000, 60000) + 8 * C;
        const int64_t Ppos = cap + std::max<int64_t>(cap / 2, (int64_t)256 * C);   // Engine::init
        const bool force32 = rnd(0, 9) == 0;
        const bool near_limit = rnd(0, 3) == 0;   // bases just below the uint16 coordinates' last Index
        const int silent_pct = (int)rnd(0, 2) * 30 + (n > 896 && (g_seq & 1) ? 25 : 0);
        std::vector<int32_t> len(C, 0), base(C, 0), len_div(C, 0), off(C + 1, 0), bm;
        std::vector<uint8_t> silent(C, 0), hot(C, 0);
        for (int c = 0; c < C; c++) {
            silent[c] = rnd(0, 99) < silent_pct;
            hot[c] = rnd(0, 15) == 0;
            if (near_limit) base[c] = (int32_t)rnd(65000, 65500);
        }
        bool laid_out = false;
        int64_t E_div = 0;
        int compact = 0;
        int32_t R = 0;
        for (g_call = 0; g_call < 10; g_call++) {
            // growth: most calls add a few events per chain, a hot chain up to several hundred (it outgrows its slot)
            int64_t En = 0;
            const int mode = (int)rnd(0, 9);   // 0: nothing grows, 1: one chain, else all but the silent
            const int only = (int)rnd(0, C - 1);
            for (int c = 0; c < C; c++) {
                int64_t add = 0;
                if (!silent[c] && mode != 0 && (mode != 1 || c == only)) add = hot[c] ? rnd(0, 400) : rnd(0, 12);
                len[c] += (int32_t)add;
                En += len[c];
            }
            if (En > cap) break;
            // a context whose chains were renumbered (a smaller first Index): the width may flip down
            if (near_limit && g_call >= 5 && rnd(0, 2) == 0)
                for (int c = 0; c < C; c++) base[c] = 0;
            const bool incremental = rnd(0, 11) != 0;
            DivideIn in{};
            in.n = n; in.G = G; in.C = C; in.Ppos = Ppos; in.En = En;
            in.chain_len = len.data(); in.chain_base = base.data();
            in.len_div = len_div.data(); in.bm = bm.data(); in.R = R;
            in.laid_out = laid_out; in.E_div = E_div; in.compact = compact;
            in.incremental = incremental; in.force_coord32 = force32; in.force_rebuild = false; in.seg = seg;
            const std::vector<int32_t> off_before = off;
            divide_plan(in, off, plan);
            calls++;
            // ---- the rules, stated directly
            bool fits16 = true;
            int max_len = 0;
            for (int c = 0; c < C; c++) {
                if (len[c] > 0 && (int64_t)base[c] + len[c] - 1 > 65533) fits16 = false;
                max_len = std::max(max_len, len[c]);
            }
            const int want_compact = (fits16 && n % 2 == 0 && !force32) ? 1 : 0;
            CHECK(plan.compact == want_compact);
            CHECK(plan.max_len == max_len);
            bool slot_short = false;
            if (laid_out)
                for (int c = 0; c < C; c++) slot_short |= len[c] > off_before[c + 1] - off_before[c];
            const bool is_first = !laid_out || E_div == 0;
            const bool flipped = want_compact != compact;
            const bool want_rebuild = is_first || flipped || !incremental || slot_short;
            CHECK(plan.rebuild == want_rebuild);
            CHECK(plan.E0 == (want_rebuild ? 0 : E_div));
            if (want_rebuild) {
                if (is_first) first++;
                else if (!incremental) inc_off++;
                else if (flipped) (want_compact ? flip_down : flip_up)++;
                else outgrown++;
                // the rebuilt layout: slots of whole 32-position blocks that hold their chains, within Ppos
                layouts++;
                CHECK((int)off.size() == C + 1 && off[0] == 0);
                for (int c = 0; c < C; c++) {
                    const int32_t slot = off[c + 1] - off[c];
                    CHECK(slot % 32 == 0);
                    CHECK(slot >= len[c]);
                }
                CHECK(off[C] <= Ppos);
                CHECK(plan.r_lo == 0 && plan.u0 == 0 && plan.max_new == max_len);
            } else {
                CHECK(off == off_before);
                int32_t r_lo = 0x7FFFFFFF, max_new = 0;
                int64_t unit = -1;
                bool grew = false, no_old = false;
                for (int c = 0; c < C; c++) {
                    max_new = std::max(max_new, len[c] - len_div[c]);
                    if (len[c] <= len_div[c]) continue;
                    grew = true;
                    const int64_t u = len_div[c] / seg;
                    if (unit < 0 || u < unit) unit = u;
                    int32_t r_c = 0;
                    if (len_div[c] == 0 || R == 0) no_old |= len_div[c] == 0;
                    else
                        for (int32_t r = 0; r <= R; r++)   // the largest r whose boundary is among the old events
                            if (bm[(size_t)r * C + c] <= len_div[c] - 1) r_c = r;
                    r_lo = std::min(r_lo, r_c);
                }
                if (!grew) r_lo = 0;
                CHECK(plan.r_lo == r_lo);
                CHECK(plan.max_new == max_new);
                if (grew) CHECK(plan.u0 == unit * C);
                else CHECK(plan.u0 >= (int64_t)((max_len + seg - 1) / seg) * C);   // beyond every unit
                if (!grew) no_growth++;
                else if (r_lo > 0) resumed_hi++;
                else if (no_old) resumed_no_old++;
            }
            // the lane map and the graphs' sizes
            int with_events = 0;
            int64_t graph_events = 0;
            for (int g = 0; g < G; g++) {
                int64_t e = 0;
                for (int c = 0; c < n; c++) e += len[(size_t)g * n + c];
                graph_events = std::max(graph_events, e);
            }
            for (int c = 0; c < C; c++) with_events += len[c] > 0;
            CHECK(plan.graph_events == graph_events);
            CHECK(plan.lane_map == (n > 896 && G == 1));
            if (plan.lane_map) {
                CHECK(plan.la_na == with_events && (int)plan.lmap.size() == with_events);
                for (int k = 0; k < with_events; k++) {
                    CHECK(len[plan.lmap[k]] > 0);
                    if (k) CHECK(plan.lmap[k] > plan.lmap[k - 1]);
                }
                CHECK(plan.lanes_fit == (with_events <= 896));
                (plan.lanes_fit ? lanes_fit : lanes_over)++;
            } else {
                CHECK(plan.la_na == n && !plan.lanes_fit && plan.lmap.empty());
            }
            // a forced rebuild (the second attempt) of the same call: a rebuild with the same widths
            if (rnd(0, 7) == 0) {
                DividePlan again;
                std::vector<int32_t> off2 = off;
                in.force_rebuild = true;
                in.compact = plan.compact;
                divide_plan(in, off2, again);
                CHECK(again.rebuild && again.E0 == 0 && again.r_lo == 0 && again.u0 == 0 && again.compact == plan.compact);
                CHECK(again.max_len == max_len && again.max_new == max_len && off2[C] <= Ppos);
            }
            // ---- what the call leaves for the next one
            len_div = len;
            E_div = En;
            laid_out = true;
            compact = plan.compact;
            R = (int32_t)rnd(0, 12);
            if (rnd(0, 5) == 0) R = 0;
            bm.assign((size_t)(R + 1) * C, 0);
            for (int c = 0; c < C; c++) {   // boundaries: 0, then non-decreasing offsets up to the chain's length
                const int32_t step = std::max<int32_t>(1, len[c] / std::max(1, R)) + 2;
                for (int32_t r = 1; r <= R; r++) {
                    const int32_t prev = bm[(size_t)(r - 1) * C + c];
                    bm[(size_t)r * C + c] = std::min<int32_t>(len[c], prev + (int32_t)rnd(0, step));
                }
            }
        }
    }
    const int combos = check_round_path();
    std::printf("%d sequences ok: %ld calls, rebuilds %ld first %ld width up %ld width down %ld outgrown %ld incremental off; "
                "resumed %ld r_lo above 0 %ld no old event %ld no growth; lane maps %ld fit %ld over; %ld layouts, "
                "%d round-path combinations\n",
                g_seq, calls, first, flip_up, flip_down, outgrown, inc_off, resumed_hi, resumed_no_old, no_growth, lanes_fit,
                lanes_over, layouts, combos);
    return 0;
}
