// Host side of the resident body store (hgx_bodystore.h): no HIP, no context.
#include "hgx_bodystore.h"

namespace hgx {

int64_t body_grow_plan(int64_t cap, int64_t need) {
    if (need < 0 || cap < 0) return -1;
    if (need <= cap) return cap;
    int64_t c = cap < kBodyMinCap ? kBodyMinCap : cap;
    while (c < need) {
        if (c > ((int64_t)1 << 61)) return -1;
        c *= 2;
    }
    return c;
}

const char* keep_bodies_check(bool have_ctx, int64_t resident_events, int64_t tx_hint, int64_t bytes_hint,
                              bool chain_sharded, bool row_sharded) {
    if (!have_ctx) return "bad arguments";
    if (tx_hint < 0 || bytes_hint < 0) return "negative hint";
    if (chain_sharded) return "not available on a chain-sharded context";
    if (row_sharded) return "not available on a row-sharded context";
    if (resident_events != 0) return "the context holds events (a fresh context, or hgx_clear first)";
    return nullptr;
}

int body_out_fits(int64_t n_tx, int64_t n_bytes, const void* tx_off, int64_t tx_cap, const void* tx_bytes,
                  int64_t bytes_cap) {
    const int64_t tc = tx_off ? tx_cap : 0, bc = tx_bytes ? bytes_cap : 0;
    return (tc < n_tx || bc < n_bytes) ? 1 : 0;
}

int64_t decimal_len(int64_t v) {
    int64_t len = v < 0 ? 1 : 0;
    // (magnitude digit by digit: INT64_MIN has no positive counterpart)
    do {
        len++;
        v /= 10;
    } while (v != 0);
    return len;
}

int64_t base64_len(int64_t bytes) { return 4 * ((bytes + 2) / 3); }

int64_t block_text_len(int64_t round_received, int32_t ntx, bool tx_nil, const int64_t* tx_off) {
    // {"RoundReceived": (17)  N  ,"Transactions": (16)  T  }\n (2)
    int64_t len = 17 + decimal_len(round_received) + 16 + 2;
    if (tx_nil && ntx <= 0) return len + 4;   // null
    len += 2;                                 // [ ]
    for (int32_t i = 0; i < ntx; i++) len += base64_len(tx_off[i + 1] - tx_off[i]) + 2 + (i ? 1 : 0);
    return len;
}

int64_t block_text_bound(int64_t count, int64_t n_tx, int64_t n_bytes) {
    // per block at most 17 + 20 + 16 + "null}\n"; per transaction quotes, a comma or "]}\n", and
    // 4 ceil(l / 3) <= 4 (l + 2) / 3 summed over the transactions
    return 59 * count + 5 * n_tx + 4 * ((n_bytes + 2 * n_tx) / 3 + 1);
}

bool block_text_fits(int64_t text_bytes) { return text_bytes >= 0 && text_bytes < kBlockTextLimit; }

}  // namespace hgx
