// Host side of the event-body front end: see hgx_bodies.h. No HIP include.
#include "hgx_bodies.h"

#include <algorithm>
#include <cstdio>

#include "hgx.h"

namespace hgx {

const char* bodies_check(const BodiesIn& ev, int64_t count, std::vector<int64_t>& txi, bool need_sig) {
    txi.assign((size_t)(count > 0 ? count : 0) + 1, 0);
    if (count <= 0) return nullptr;
    if (!ev.creator || !ev.index || !ev.sp || !ev.op || !ev.ts || (need_sig && (!ev.r || !ev.s)) || !ev.ntx || !ev.tx_off)
        return "null column";
    int64_t t = 0;
    for (int64_t k = 0; k < count; k++) {
        if (ev.ntx[k] < -1) return "ntx below -1";
        txi[(size_t)k] = t;
        t += ev.ntx[k] > 0 ? ev.ntx[k] : 0;
    }
    txi[(size_t)count] = t;
    if (ev.tx_off[0] < 0) return "negative tx_off";
    for (int64_t j = 0; j < t; j++)
        if (ev.tx_off[j + 1] < ev.tx_off[j]) return "tx_off must be non-decreasing";
    if (ev.tx_off[t] > ev.tx_off[0] && !ev.tx_bytes) return "null tx_bytes";
    return nullptr;
}

int64_t batch_levels(const int64_t* sp, const int64_t* op, int64_t count, int64_t base, int32_t* level,
                     int32_t* n_levels) {
    int32_t top = 0;
    for (int64_t k = 0; k < count; k++) {
        const int64_t g = base + k;
        if (sp[k] >= g || op[k] >= g) return k;
        int32_t l = 0;
        if (sp[k] >= base) l = level[sp[k] - base] + 1;
        if (op[k] >= base) l = std::max(l, level[op[k] - base] + 1);
        level[k] = l;
        top = std::max(top, l + 1);
    }
    if (n_levels) *n_levels = top;
    return -1;
}

int64_t bodies_first_unencodable(const BodiesIn& ev, int64_t count, int64_t base, int32_t n_keys,
                                 const uint8_t* root_has_y, bool have_op_ids) {
    for (int64_t k = 0; k < count; k++) {
        const int64_t g = base + k;
        if (ev.creator[k] < 0 || ev.creator[k] >= n_keys || ev.sp[k] < -1 || ev.sp[k] >= g || ev.op[k] >= g) return k;
        if (ev.op[k] < -1) {
            const bool has_text = root_has_y && ((ev.op[k] == HGX_ROOT_Y && root_has_y[ev.creator[k]]) ||
                                                 (ev.op[k] == HGX_ROOT_OTHER && have_op_ids));
            if (!has_text) return k;
        }
    }
    return count;
}

int64_t bodies_chunk_end(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t lo, int64_t hi,
                         int64_t* bound) {
    int64_t sum = 0, k = lo;
    for (; k < hi && k - lo < kBodyChunkEvents; k++) {
        int64_t b = kBodyFixedBytes;
        for (int64_t j = txi[(size_t)k]; j < txi[(size_t)k + 1]; j++)
            b += 4 * ((ev.tx_off[j + 1] - ev.tx_off[j] + 2) / 3) + 8;   // (3 of text; 8 bound the offsets' share)
        b = (b + 15) & ~(int64_t)15;
        if (k > lo && sum + b > kBodyChunkBytes) break;
        sum += b;
    }
    *bound = sum;
    return k;
}

void plan_levels(const int32_t* creator, const int32_t* level, int64_t count, int32_t n_per_graph, LevelPlan& plan) {
    plan = LevelPlan();
    if (count <= 0) return;
    int32_t top_graph = 0;
    for (int64_t k = 0; k < count; k++) top_graph = std::max(top_graph, creator[k] / n_per_graph);
    // levels of every graph present in the chunk, then one workgroup per such graph
    std::vector<int32_t> g_nl((size_t)top_graph + 1, 0), g_slot((size_t)top_graph + 1, -1);
    for (int64_t k = 0; k < count; k++) {
        int32_t& nl = g_nl[(size_t)(creator[k] / n_per_graph)];
        nl = std::max(nl, level[k] + 1);
    }
    int32_t lo = 0;
    for (int32_t g = 0; g <= top_graph; g++) {
        if (!g_nl[(size_t)g]) continue;
        g_slot[(size_t)g] = (int32_t)plan.wg_lo.size();
        plan.wg_lo.push_back(lo);
        plan.wg_nl.push_back(g_nl[(size_t)g]);
        lo += g_nl[(size_t)g] + 1;
    }
    plan.loff.assign((size_t)lo, 0);
    // counting sort by (workgroup, level): counts into the slot after each level's start
    for (int64_t k = 0; k < count; k++)
        plan.loff[(size_t)(plan.wg_lo[(size_t)g_slot[(size_t)(creator[k] / n_per_graph)]] + level[k] + 1)]++;
    int32_t run = 0;
    for (size_t j = 0; j < plan.wg_lo.size(); j++) {
        const size_t a = (size_t)plan.wg_lo[j];
        plan.loff[a] = run;
        for (int32_t l = 1; l <= plan.wg_nl[j]; l++) {
            plan.max_width = std::max(plan.max_width, plan.loff[a + (size_t)l]);
            run += plan.loff[a + (size_t)l];
            plan.loff[a + (size_t)l] = run;
        }
    }
    plan.pos.assign((size_t)count, 0);
    std::vector<int32_t> cur(plan.loff);
    for (int64_t k = 0; k < count; k++) {
        const size_t a = (size_t)(plan.wg_lo[(size_t)g_slot[(size_t)(creator[k] / n_per_graph)]] + level[k]);
        plan.pos[(size_t)cur[a]++] = (int32_t)k;
    }
}

}  // namespace hgx

extern "C" int32_t hgx_batch_levels(const int64_t* self_parent, const int64_t* other_parent, int64_t count,
                                    int64_t base, int32_t* level, int32_t* n_levels, hgx_error* err) {
    auto fail = [&](const char* msg) {
        if (err) {
            err->code = HGX_ERR_INVALID;
            std::snprintf(err->msg, sizeof(err->msg), "%s", msg);
        }
        return (int32_t)HGX_ERR_INVALID;
    };
    if (n_levels) *n_levels = 0;
    if (count < 0 || base < 0 || (count > 0 && (!self_parent || !other_parent || !level)))
        return fail("hgx_batch_levels: bad arguments");
    const int64_t bad = hgx::batch_levels(self_parent, other_parent, count, base, level, n_levels);
    if (bad >= 0) {
        char msg[128];
        std::snprintf(msg, sizeof(msg), "hgx_batch_levels: event %lld names a parent that is not an earlier event",
                      (long long)bad);
        return fail(msg);
    }
    if (err) {
        err->code = HGX_OK;
        err->msg[0] = 0;
    }
    return HGX_OK;
}
