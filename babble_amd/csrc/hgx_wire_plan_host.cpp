// Host plan of hgx_insert_wire_bodies (hgx_wire_plan.h): no HIP, no context.
#include "hgx_wire_plan.h"

#include <algorithm>

#include "hgx.h"

namespace hgx {

std::string wire_go_rune(int64_t v) {
    uint32_t r = (v < 0 || v > 0x10FFFF || (v >= 0xD800 && v <= 0xDFFF)) ? 0xFFFD : (uint32_t)v;
    std::string s;
    if (r < 0x80) s += (char)r;
    else if (r < 0x800) { s += (char)(0xC0 | (r >> 6)); s += (char)(0x80 | (r & 63)); }
    else if (r < 0x10000) { s += (char)(0xE0 | (r >> 12)); s += (char)(0x80 | ((r >> 6) & 63)); s += (char)(0x80 | (r & 63)); }
    else { s += (char)(0xF0 | (r >> 18)); s += (char)(0x80 | ((r >> 12) & 63)); s += (char)(0x80 | ((r >> 6) & 63)); s += (char)(0x80 | (r & 63)); }
    return s;
}

void wire_plan(const WireIn& w, int64_t count, const int32_t* last_index, const int32_t* chain_len, int n, int64_t E0,
               WirePlan& plan) {
    plan = WirePlan();
    const size_t nz = (size_t)(n > 0 ? n : 0), cz = (size_t)(count > 0 ? count : 0);
    plan.lo.assign(nz, kWireNoWindow);
    plan.woff.assign(nz, 0);
    plan.sp.reserve(cz);
    plan.op.reserve(cz);
    plan.level.reserve(cz);
    // the batch's events per creator, in batch order: pend[poff[c] .. poff[c] + pcnt[c]) = their positions
    std::vector<int64_t> poff(nz + 1, 0), pcnt(nz, 0), pend(cz);
    for (size_t k = 0; k < cz; k++)
        if (w.creator[k] >= 0 && w.creator[k] < n) poff[(size_t)w.creator[k] + 1]++;
    for (size_t c = 0; c < nz; c++) poff[c + 1] += poff[c];
    // Store.ParticipantEvent(p, idx): 0 none of the errors, d = the descriptor; a resident event's
    // descriptor holds its Index for now (-2 - Index), the window slot once every lo[] is known
    auto participant_event = [&](int32_t p, int64_t idx, int64_t* d) -> int32_t {
        if (p < 0 || p >= n) {   // ReverseParticipants miss: participantEvents[""] is nil
            plan.msg = "runtime error: invalid memory address or nil pointer dereference";
            return HGX_ERR_PANIC;
        }
        const int64_t np = pcnt[(size_t)p], cl = chain_len[p];
        const int64_t items = cl + np;
        const int64_t last = np ? w.index[pend[(size_t)(poff[(size_t)p] + np - 1)]] : (int64_t)last_index[p];
        const int64_t oldest = last - items + 1;
        if (idx < oldest) { plan.msg = wire_go_rune(idx) + ", Too Late"; return HGX_ERR_TOO_LATE; }
        const int64_t f = idx - oldest;
        if (f >= items) { plan.msg = wire_go_rune(idx) + ", Not Found"; return HGX_ERR_KEY_NOT_FOUND; }
        if (f >= cl) {
            *d = E0 + pend[(size_t)(poff[(size_t)p] + f - cl)];
        } else {   // the resident chain holds consecutive Indexes: position f is Index (last - len + 1) + f
            *d = -2 - ((int64_t)last_index[p] - cl + 1 + f);
        }
        return HGX_OK;
    };
    auto name_resident = [&](int32_t p, int64_t d) {   // (only parents of the prefix open a window)
        if (d > -2) return;
        plan.lo[(size_t)p] = (int32_t)std::min<int64_t>(plan.lo[(size_t)p], -2 - d);
        plan.n_resident++;
    };
    plan.m = count > 0 ? count : 0;
    for (int64_t k = 0; k < count; k++) {
        const int32_t cr = w.creator[k];
        int32_t rc = HGX_OK;
        int64_t s = -1, o = -1;
        if (cr < 0 || cr >= n) {   // creator[2:] of "" (hashgraph.go:578-582)
            rc = HGX_ERR_PANIC;
            plan.msg = "runtime error: slice bounds out of range [2:0]";
        }
        if (rc == HGX_OK && w.spi[k] >= 0) rc = participant_event(cr, w.spi[k], &s);
        if (rc == HGX_OK && w.opi[k] >= 0) rc = participant_event(w.opc[k], w.opi[k], &o);
        if (rc != HGX_OK) {
            plan.m = k;
            plan.code = rc;
            break;
        }
        name_resident(cr, s);
        if (o <= -2) name_resident(w.opc[k], o);
        int32_t l = 0;
        if (s >= 0) l = plan.level[(size_t)(s - E0)] + 1;
        if (o >= 0) l = std::max(l, plan.level[(size_t)(o - E0)] + 1);
        plan.sp.push_back(s);
        plan.op.push_back(o);
        plan.level.push_back(l);
        plan.n_levels = std::max(plan.n_levels, l + 1);
        pend[(size_t)(poff[(size_t)cr] + pcnt[(size_t)cr]++)] = k;
    }
    // the windows: [lo[c], last_index[c]] of every named creator, one after the other
    for (size_t c = 0; c < nz; c++) {
        plan.woff[c] = (int32_t)plan.slots;
        if (plan.lo[c] != kWireNoWindow) plan.slots += (int64_t)last_index[c] - plan.lo[c] + 1;
    }
    if (!plan.n_resident) return;
    for (int64_t k = 0; k < plan.m; k++) {
        int64_t& s = plan.sp[(size_t)k];
        if (s <= -2) {
            const size_t c = (size_t)w.creator[k];
            s = -2 - ((int64_t)plan.woff[c] + (-2 - s) - plan.lo[c]);
        }
        int64_t& o = plan.op[(size_t)k];
        if (o <= -2) {
            const size_t c = (size_t)w.opc[k];
            o = -2 - ((int64_t)plan.woff[c] + (-2 - o) - plan.lo[c]);
        }
    }
}

}  // namespace hgx
