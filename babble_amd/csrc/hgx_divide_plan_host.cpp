// Host plan of DivideRounds (hgx_divide_plan.h): no HIP, no context.
#include "hgx_divide_plan.h"

#include <algorithm>

namespace hgx {

void layout_slots(int C, int64_t Ppos, int64_t En, const int32_t* chain_len, std::vector<int32_t>& off) {
    int act = 0;
    for (int c = 0; c < C; c++) act += chain_len[c] > 0 ? 1 : 0;
    const int64_t share = (Ppos - En) / (2 * (int64_t)act + (C - act));
    off.assign((size_t)C + 1, 0);
    // slots of multiples of 32 positions (a share >= 128 > 31: Ppos >= capacity + 256 C): every
    // chain starts 64-byte aligned in the firstDescendants columns (the round kernels' staging)
    for (int c = 0; c < C; c++)
        off[c + 1] = off[c] + ((chain_len[c] + (int32_t)((chain_len[c] > 0 ? 2 : 1) * share)) & ~31);
}

void divide_plan(const DivideIn& in, std::vector<int32_t>& off, DividePlan& p) {
    const int C = in.C;
    int32_t max_index = -1;
    p.max_len = 0;
    for (int c = 0; c < C; c++) {
        if (in.chain_len[c] > 0) max_index = std::max(max_index, in.chain_base[c] + in.chain_len[c] - 1);
        p.max_len = std::max(p.max_len, in.chain_len[c]);
    }
    p.compact = (!in.force_coord32 && (in.n % 2) == 0 && max_index <= kCoord16Max) ? 1 : 0;
    p.rebuild = in.force_rebuild || !in.laid_out || in.E_div == 0 || p.compact != in.compact || !in.incremental;
    if (!p.rebuild)
        for (int c = 0; c < C; c++)
            if (in.chain_len[c] > off[c + 1] - off[c]) { p.rebuild = true; break; }
    p.E0 = p.rebuild ? 0 : in.E_div;
    p.r_lo = 0;
    p.u0 = 0;
    p.max_new = p.max_len;
    if (p.rebuild) {
        layout_slots(C, in.Ppos, in.En, in.chain_len, off);
    } else {
        int32_t r_lo = 0x7FFFFFFF, smin = 0x7FFFFFFF;
        p.max_new = 0;
        for (int c = 0; c < C; c++) {
            p.max_new = std::max(p.max_new, in.chain_len[c] - in.len_div[c]);
            if (in.chain_len[c] <= in.len_div[c]) continue;
            smin = std::min(smin, in.len_div[c] / in.seg);
            const int32_t last = in.len_div[c] - 1;
            if (last < 0 || in.R == 0) { r_lo = 0; continue; }
            if (r_lo == 0) continue;
            int32_t lo = 0, hi = in.R;   // largest r in [0, R] with bm[r][c] <= last
            while (lo < hi) {
                const int32_t mid = (lo + hi + 1) / 2;
                if (in.bm[(size_t)mid * C + c] <= last) lo = mid; else hi = mid - 1;
            }
            r_lo = std::min(r_lo, lo);
        }
        p.r_lo = r_lo == 0x7FFFFFFF ? 0 : r_lo;
        p.u0 = (int64_t)smin * C;
    }
    p.lane_map = in.n > kLaLanes && in.G == 1;
    p.la_na = in.n;
    p.lmap.clear();
    if (p.lane_map) {
        for (int c = 0; c < C; c++)
            if (in.chain_len[c] > 0) p.lmap.push_back(c);
        p.la_na = (int)p.lmap.size();
    }
    p.lanes_fit = p.lane_map && p.la_na <= kLaLanes;
    p.graph_events = 0;
    for (int g = 0; g < in.G; g++) {
        int64_t e = 0;
        for (int c = 0; c < in.n; c++) e += in.chain_len[(size_t)g * in.n + c];
        p.graph_events = std::max(p.graph_events, e);
    }
}

RoundChoice round_path(const RoundPathIn& in) {
    RoundChoice rc{};
    const int k = in.round_kernel;
    // the persistent launch pays a fixed cost (every chain's window staged, 256 resident workgroups)
    // that a call resuming for a few rounds does not recover: those use the steps (a chain-sharded
    // group always runs it: its shards build firstDescendants for their own chains only)
    if (!in.rooted && in.g_ok && (k == 0 || k == 4) && !in.sharded) rc.path = RoundPath::WholeGraph;
    else if (!in.rooted && (k == 3 || (k == 0 && in.rebuild) || in.sharded) &&
             (in.p_ok || (in.pb_ok && !in.sharded && in.round_pb_enabled)))
        rc.path = in.p_ok ? RoundPath::Persistent : RoundPath::PersistentBig;   // (p_ok: n <= 256, pb_ok: n > 256)
    else rc.path = RoundPath::Steps;
    // the resumed calls that follow such a rebuild use the per-launch steps
    rc.precapture = (rc.path == RoundPath::Persistent || rc.path == RoundPath::PersistentBig) && in.rebuild && k == 0;
    rc.step_kernel = (in.rooted || k != 1) ? 0 : 1;   // root floors: per-candidate step only
    // a rebuild replays kStepBatch steps per hipGraph; a resumed call (a few rounds) 2 or 4: a
    // round holds ~10-14 events per chain, so fewer than 6 new events per chain rarely take
    // more than two steps (a second batch costs another host round trip)
    const bool few = in.new_events < 6 * (int64_t)in.C;
    rc.step_graph = in.rebuild ? 0 : few ? 1 : 2;
    rc.nb = in.rebuild ? kStepBatch : few ? kStepBatchSmall : 2 * kStepBatchSmall;
    return rc;
}

}  // namespace hgx
