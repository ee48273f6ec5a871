// Version-3 checkpoint files (hgx_save_bodies / hgx_bootstrap, include/hgx.h "persistence", DESIGN.md
// §3.17): the section parser, the validator and the piece planner of the replay. Plain C++ with no HIP
// include and no context (hgx_ckpt_host.cpp), so tools/ckpt_host_check.cpp runs them as a program of its
// own under the host sanitizers. The version 1 / 2 reader stays in hgx_api.cpp.
//
// Nothing here copies a section: a parsed image is a set of byte pointers into the caller's buffer, read
// through ckpt_rd (the sections are not aligned for their element types).
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace hgx {

enum : int32_t { kCkRooted = 1, kCkIds = 2, kCkKeys = 4, kCkPayloads = 8, kCkBodies = 16 };
constexpr uint64_t kFnvBasis = 14695981039346656037ull, kFnvPrime = 1099511628211ull;
constexpr size_t kCkptHeaderBytes = 32, kCkptBlockBytes = 24, kCkptBlockHashBytes = 36;

template <typename T>
inline T ckpt_rd(const uint8_t* p, int64_t i = 0) {
    T v;
    std::memcpy(&v, p + (size_t)i * sizeof(T), sizeof(T));
    return v;
}

// What Reset kept of one graph (the rooted section)
struct Ckpt3Kept {
    int32_t has_lcr = 0, lcr = 0, lcre = 0;
    int64_t consensus_tx = 0, n_blocks = 0;
    const uint8_t* blocks = nullptr;   // n_blocks x (i32 rr, i32 events, i64 transactions, i32 nil, i32 committed)
    const uint8_t* hashes = nullptr;   // n_blocks x (u8 has_hash, 3 zero bytes, u8 hash[32])
};

// A validated version-3 image: every pointer and count below lies inside [buf, buf + len - 8)
struct Ckpt3 {
    int32_t n = 0, G = 0, flags = 0;
    int64_t E = 0, C = 0;
    // rooted files (flags & kCkRooted), else null / 0
    const uint8_t *root_index = nullptr, *root_round = nullptr, *root_y = nullptr;   // i32[C], i32[C], u8[C]
    int64_t n_others = 0;
    const uint8_t* others = nullptr;                                                  // [n_others][32]
    std::vector<Ckpt3Kept> kept;                                                      // [G]
    const uint8_t *has_x = nullptr, *has_y = nullptr, *x_id = nullptr, *y_id = nullptr;   // u8[C], u8[C], [C][32] x 2
    int64_t n_pairs = 0;
    const uint8_t *pair_event = nullptr, *pair_parent = nullptr;                      // [n_pairs][32], sorted by event
    // the events (gid order)
    const uint8_t *creator = nullptr, *index = nullptr, *sp = nullptr, *op = nullptr, *ts = nullptr;   // i32, i64 x 4
    const uint8_t *sig_s = nullptr, *coin = nullptr, *ntx = nullptr, *nil = nullptr;   // [E][32], u8, i32, u8
    const uint8_t *ids = nullptr, *keys = nullptr, *sig_r = nullptr;                   // [E][32], [C][65], [E][32]
    int64_t T = 0, n_bytes = 0;
    const uint8_t *tx_off = nullptr, *tx_bytes = nullptr;                             // i64[T + 1], u8[n_bytes]
};

// FNV-1a over [p, p + n), continued from h
uint64_t ckpt_fnv1a(uint64_t h, const void* p, size_t n);

// Parse and validate a whole version-3 file image (its closing checksum included). Null = accepted and
// `out` filled; else the reason, worded as hgx_bootstrap reports it behind "hgx_bootstrap: " ("truncated
// file", "checksum mismatch", "size mismatch", "unsupported flags", "T is not the sum of ntx", ...).
// want_n / want_G: the context's shape (0 = any). Reads nothing outside [buf, buf + len).
const char* ckpt3_parse(const uint8_t* buf, size_t len, int32_t want_n, int32_t want_G, Ckpt3& out, std::string& why);

// The replay's pieces: events [lo, *hi) with transactions [t_lo, *t_hi) is the longest run from lo of at
// most max_events events whose transaction bytes stay within max_bytes, cut at an event boundary; a
// single event larger than max_bytes is a piece of its own. t_lo = the first transaction of event lo
// (the sum of ntx below lo). lo in [0, E), max_events >= 1.
void ckpt3_piece(const Ckpt3& f, int64_t lo, int64_t t_lo, int64_t max_events, int64_t max_bytes, int64_t* hi,
                 int64_t* t_hi);

// The row of the sorted pairs whose event id is id32, or -1
int64_t ckpt3_find_pair(const Ckpt3& f, const uint8_t* id32);

}  // namespace hgx
