// Host plan of hgx_diff_wire (hgx_diff.h): no HIP, no context.
#include "hgx_diff.h"

namespace hgx {

void diff_plan(const int32_t* known, const int32_t* last_index, const int32_t* chain_len, int n, int64_t sync_limit,
               DiffPlan& plan) {
    plan = DiffPlan();
    plan.count.assign((size_t)(n > 0 ? n : 0), 0);
    // Core.OverSyncLimit (node/core.go:147-159)
    for (int i = 0; i < n; i++) {
        const int64_t li = last_index[i], kn = known[i];
        if (li > kn) plan.unknown += li - kn;
    }
    if (sync_limit >= 0 && plan.unknown > sync_limit) {
        plan.over_limit = true;
        return;
    }
    // Core.Diff (node/core.go:166-188): Store.ParticipantEvents(pk, known[id]) per participant
    for (int i = 0; i < n; i++) {
        const int64_t last = last_index[i], items = chain_len[i], skip = known[i];
        if (skip > last) continue;                 // RollingIndex.Get (common/rolling_index.go:24-26)
        const int64_t oldest = last - items + 1;
        if (skip + 1 < oldest) {                   // NewStoreErr(TooLate, string(SkippedIndex))
            plan.fail = i;
            plan.msg = std::string("\x03") + ", Too Late";
            plan.total = 0;
            plan.count.assign((size_t)n, 0);
            return;
        }
        const int64_t start = skip - oldest + 1;
        plan.count[(size_t)i] = items - start;
        plan.total += items - start;
    }
}

}  // namespace hgx
