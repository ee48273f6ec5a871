// Host plan of hgx_insert_wire_bodies: ReadWireInfo (hashgraph.go:569-614) for a
// whole SyncResponse, decided from the per-chain tables the context already mirrors. Plain C++ with
// no HIP include (hgx_wire_plan_host.cpp), so a stand-alone program can run it under the host
// sanitizers; the device side is hgx_wire.hip.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace hgx {

// the wire columns the plan reads (hgx_wire_bodies' first five)
struct WireIn {
    const int32_t* creator;
    const int64_t *index, *spi;
    const int32_t* opc;
    const int64_t* opi;
};

constexpr int32_t kWireNoWindow = 0x7FFFFFFF;   // lo[c] of a creator whose resident events nobody names

// A parent descriptor (sp / op, one per event before the first resolution error):
//   -1          no parent ("")
//   >= 0        final gid E0 + k' of the batch's event at position k'
//   <= -2       resident event, window slot -2 - d: its gid is win[slot] once k_wire_window ran
// The two columns go to the device as the body path's parent columns; k_wire_resolve replaces the
// window descriptors by gids in place before anything else reads them.
struct WirePlan {
    int64_t m = 0;                  // events before the first resolution error (count when there is none)
    int32_t code = 0;               // that error: HGX_ERR_TOO_LATE / _KEY_NOT_FOUND / _PANIC, or HGX_OK
    std::string msg;                // ... with the Go error string
    std::vector<int64_t> sp, op;    // [m] parent descriptors
    std::vector<int32_t> level;     // [m] depth inside the batch: in-batch parent's level + 1, resident parent 0
    int32_t n_levels = 0;
    std::vector<int32_t> lo, woff;  // [n] smallest resident Index named / first window slot of each creator
    int64_t slots = 0;              // window slots in all: sum over named creators of last_index - lo + 1
    int64_t n_resident = 0;         // parents that are resident events (0: no window launch)
};

// count events of n participants against a context with E0 resident events whose chain c holds
// chain_len[c] events ending at Index last_index[c] (Store.ParticipantEvent over RollingIndex.GetItem,
// common/rolling_index.go:40-50, positional; the batch's earlier events count as inserted). O(count + n).
void wire_plan(const WireIn& w, int64_t count, const int32_t* last_index, const int32_t* chain_len, int n, int64_t E0,
               WirePlan& plan);

// Go's string(int): UTF-8 of the rune (common/rolling_index.go passes string(index))
std::string wire_go_rune(int64_t v);

}  // namespace hgx
