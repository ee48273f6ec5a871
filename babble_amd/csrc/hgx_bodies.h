// Host side of the event-body front end (hgx_insert_event_bodies / hgx_event_json_batch,
// DESIGN.md §3.10): argument checks, the batch's dependency levels and the chunk plan. Plain C++
// with no HIP include (hgx_bodies_host.cpp), so a stand-alone program can run it under the host
// sanitizers; the device side is hgx_goenc_dev.hip.
#pragma once

#include <cstdint>
#include <vector>

namespace hgx {

// hgx_event_bodies' columns (host pointers)
struct BodiesIn {
    const int32_t* creator;
    const int64_t *index, *sp, *op, *ts;
    const uint8_t *r, *s;
    const int32_t* ntx;
    const int64_t* tx_off;
    const uint8_t* tx_bytes;
};

constexpr int64_t kBodyChunkEvents = 65536;        // events per internal chunk, at most
constexpr int64_t kBodyChunkBytes = 32ll << 20;    // JSON bytes per internal chunk (one event may exceed it)
constexpr int64_t kBodyFixedBytes = 576;           // bound of an event's JSON without its transactions, padded

// nullptr if the columns are usable, else what is wrong with them. txi (count + 1 entries) gets each
// event's first entry of tx_off (the running sum of max(ntx, 0)). need_sig = false: the r and s columns
// may be null (the signing path, where the device computes both).
const char* bodies_check(const BodiesIn& ev, int64_t count, std::vector<int64_t>& txi, bool need_sig = true);

// An event's depth inside the batch whose first event has gid `base`: 0 when no parent has gid >=
// base, else 1 + the maximum over its in-batch parents. Returns -1, or the position of the first
// event with a parent gid >= its own gid (level is then not complete).
int64_t batch_levels(const int64_t* sp, const int64_t* op, int64_t count, int64_t base, int32_t* level,
                     int32_t* n_levels);

// The first position whose event has no Go-JSON text: a creator outside [0, n_keys) or a parent that
// is neither -1 nor an earlier gid (count if there is none). On a context with root ids (root_has_y
// not null: [n_keys] flags) two other-parent codes have a text as well: HGX_ROOT_Y
// where the creator's root has a Y, and HGX_ROOT_OTHER when the caller supplied the ids (have_op_ids).
int64_t bodies_first_unencodable(const BodiesIn& ev, int64_t count, int64_t base, int32_t n_keys,
                                 const uint8_t* root_has_y = nullptr, bool have_op_ids = false);

// One past the last event of the chunk that starts at lo: at most kBodyChunkEvents events and
// kBodyChunkBytes of JSON by the per-event bound (at least one event). *bound = the chunk's bound with
// every text padded to 16 bytes.
int64_t bodies_chunk_end(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t lo, int64_t hi,
                         int64_t* bound);

// Chunk positions grouped by (graph, level) with a counting sort: workgroup j of the id pass owns the
// levels loff[wg_lo[j] .. wg_lo[j] + wg_nl[j]] (wg_nl[j] + 1 offsets into pos). max_width = the widest
// level of any graph.
struct LevelPlan {
    std::vector<int32_t> pos, loff, wg_lo, wg_nl;
    int32_t max_width = 0;
};
void plan_levels(const int32_t* creator, const int32_t* level, int64_t count, int32_t n_per_graph, LevelPlan& plan);

}  // namespace hgx
