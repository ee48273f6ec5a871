// The resident body store (hgx_keep_bodies): what the host decides. No HIP, no
// context: growth plan, capacity and argument checks, the block-text sizing formula
// (hgx_bodystore_host.cpp; tools/bodystore_host_check.cpp checks them as a program of its own).
#pragma once

#include <cstdint>

namespace hgx {

// Store states (hgx_bodies_state)
enum { kBodiesOff = 0, kBodiesComplete = 1, kBodiesLost = 2 };

// The capacity a table of `cap` entries grows to so that `need` entries fit: cap itself while it
// holds them, else doublings of max(cap, kBodyMinCap) until it does (at most one allocation and one
// copy per chunk). -1: need is negative or the doubling would pass 2^62.
constexpr int64_t kBodyMinCap = 1024;
int64_t body_grow_plan(int64_t cap, int64_t need);

// hgx_keep_bodies' argument check: the reason it is refused, or null
const char* keep_bodies_check(bool have_ctx, int64_t resident_events, int64_t tx_hint, int64_t bytes_hint,
                              bool chain_sharded, bool row_sharded);

// The read-back rule of hgx_get_event_bodies, hgx_block_transactions and hgx_diff_wire_bodies: the
// totals are always reported; the arrays are written only when both fit
// (0 fits, 1 HGX_ERR_CAPACITY). A NULL array has capacity 0.
int body_out_fits(int64_t n_tx, int64_t n_bytes, const void* tx_off, int64_t tx_cap, const void* tx_bytes,
                  int64_t bytes_cap);

// Length of json.NewEncoder.Encode(&Block) (block.go:44-53): {"RoundReceived":N,"Transactions":T}\n,
// T = null for a nil list without transactions, else [ "base64", ... ]; tx_off: ntx + 1 offsets.
int64_t decimal_len(int64_t v);
int64_t base64_len(int64_t bytes);   // std encoding, padded: 4 ceil(len / 3)
int64_t block_text_len(int64_t round_received, int32_t ntx, bool tx_nil, const int64_t* tx_off);
// The block encoder's positions are 32-bit (hgx_goenc_dev.hip): the text of one batch stays below
// 4 GiB, which the host decides in 64 bits before anything is launched. hgx_block_hash_batch has the
// offsets and sums block_text_len; hgx_find_order has only the gather's totals and uses the bound,
// which is never less than that sum for `count` blocks of n_tx transactions and n_bytes bytes.
constexpr int64_t kBlockTextLimit = (int64_t)1 << 32;
int64_t block_text_bound(int64_t count, int64_t n_tx, int64_t n_bytes);
bool block_text_fits(int64_t text_bytes);

}  // namespace hgx
