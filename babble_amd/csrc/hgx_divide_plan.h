// Host plan of DivideRounds: what a call decides before its first launch -- the
// coordinate width, rebuild or resume, the lowest round that can change, the first dirty
// lastAncestors unit, the lane map above 896 chains -- and which round recurrence runs. Plain C++
// with no HIP include (hgx_divide_plan_host.cpp), so a stand-alone program can run it under the
// host sanitizers (tools/divide_plan_check.cpp); the calls that use it are in hgx_engine_divide.cpp.
#pragma once

#include <cstdint>
#include <vector>

namespace hgx {

constexpr int kStepBatch = 16;        // round steps per hipGraph replay (a full DivideRounds)
constexpr int kStepBatchSmall = 2;    // ... when resuming at the lowest changed round
constexpr int kLaLanes = 896;         // chains a k_la_wave workgroup can give a lane each
constexpr int32_t kCoord16Max = 65533;   // largest Index below Coord<uint16_t>'s sentinels (hgx_device.h)

// The slots of a rebuilt layout: off[c + 1] - off[c] positions for chain c, its events plus slack in
// shares: two for a chain with events, one for a chain without (a silent peer, or one that has not
// created an event yet). With even shares c5's 341 silent peers held a third of the slack and the
// live chains outgrew theirs two thirds through the run (an 18.8 ms rebuild call).
void layout_slots(int C, int64_t Ppos, int64_t En, const int32_t* chain_len, std::vector<int32_t>& off);

struct DivideIn {
    int n, G, C;
    int64_t Ppos, En;
    const int32_t *chain_len, *chain_base;   // [C] now
    // the previous call's state (read only while laid_out and E_div > 0)
    const int32_t* len_div;   // [C] chain lengths
    const int32_t* bm;        // [(R + 1) x C] round boundaries
    int32_t R;
    bool laid_out;
    int64_t E_div;
    int compact;
    bool incremental, force_coord32;
    bool force_rebuild;       // the second attempt of a call whose wavefront gave up
    int seg;                  // rows per lastAncestors unit
};

struct DividePlan {
    int compact = 0;          // uint16 coordinates: every Index fits below the sentinels and rows are whole dwords
    bool rebuild = false;     // the layout is rebuilt and everything recomputed (off holds the new slots)
    int64_t E0 = 0;           // events that keep their rows: 0 on a rebuild, else the previous call's
    int max_len = 0;          // longest chain
    int max_new = 0;          // most new events of one chain (a rebuild: max_len)
    // first round whose step can change: the lowest round of the last old event of a chain that got
    // new events (every boundary below it is among old events). 0 on a rebuild, when such a chain had
    // no old event, when R == 0, and when no chain grew.
    int32_t r_lo = 0;
    // first dirty lastAncestors unit of a resumed call: C x the lowest unit row of a grown chain's
    // first new event (beyond every unit when no chain grew); 0 on a rebuild
    int64_t u0 = 0;
    // n > kLaLanes, one graph: lanes for the chains that have events only (silent peers have none)
    bool lane_map = false;    // lmap / la_na are set
    bool lanes_fit = false;   // ... and fit a workgroup
    int la_na = 0;            // lanes wanted: n without a map
    std::vector<int32_t> lmap;
    int64_t graph_events = 0; // most events of one graph (the small-graph kernel's LDS size)
};

// off: the previous layout's slots ([C + 1], read unless the call rebuilds for another reason);
// a rebuild overwrites it with layout_slots'. plan is reused across calls (its vector keeps its capacity).
void divide_plan(const DivideIn& in, std::vector<int32_t>& off, DividePlan& plan);

enum class RoundPath { WholeGraph, Persistent, PersistentBig, Steps };

struct RoundPathIn {
    int round_kernel;         // hgx_set_round_kernel
    bool rooted, sharded, rebuild, round_pb_enabled;
    bool g_ok, p_ok, pb_ok;   // round_g_ok / round_p_ok / round_pb_ok for this context
    int64_t new_events;       // En - E0
    int C;
};

struct RoundChoice {
    RoundPath path;           // what runs first; a persistent launch that gives up falls back to the steps
    bool precapture;          // a rebuild whose resumed calls will step: their hipGraphs are captured now
    int step_kernel;          // 0 per-candidate, 1 block-search
    int step_graph;           // which captured batch: 0 rebuild, 1 / 2 resumed
    int nb;                   // steps per replay
};

RoundChoice round_path(const RoundPathIn& in);

}  // namespace hgx
