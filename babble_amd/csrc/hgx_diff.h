// Host plan of hgx_diff_wire: Core.OverSyncLimit and the sizes of Core.Diff
// (node/core.go:147-188) from the per-chain tables the context already mirrors. Plain C++ with no
// HIP include (hgx_diff_host.cpp), so a stand-alone program can run it under the host sanitizers;
// the device side is hgx_diff.hip.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace hgx {

struct DiffPlan {
    std::vector<int64_t> count;   // [n] events of each chain with Index > known
    int64_t total = 0;            // their sum: the rows of the response
    bool over_limit = false;      // OverSyncLimit: nothing else is filled in
    int64_t unknown = 0;          // OverSyncLimit's totUnknown
    int fail = -1;                // the first participant (ascending id) whose window refuses `known`
    std::string msg;              // ... with the Go error string ("\x03, Too Late")
};

// known / last_index / chain_len: n entries each (last_index -1 and chain_len 0 for a chain without
// events). sync_limit < 0: no limit. Per chain the window rule of RollingIndex.Get
// (common/rolling_index.go:21-39): nothing when known > last, "Too Late" when known + 1 < oldest =
// last - len + 1, else the events from Index known + 1 on.
void diff_plan(const int32_t* known, const int32_t* last_index, const int32_t* chain_len, int n, int64_t sync_limit,
               DiffPlan& plan);

}  // namespace hgx
